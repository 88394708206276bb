"""Pass groups on the device (execute_stage in h264decode_amd/csrc/mi_batch.cpp): small CABAC I/P batches with the group size forced through
h264mi_internal_set_pass_group -- short test streams never oversubscribe the chip, so the plan would leave them alone -- and the route asserted
through h264mi_internal_pass_waits.  Seven executes back to back over two prepared batches used alternately (seven is a multiple of neither group
size), one sync; the frames of the last two passes against the ungrouped run and the oracle, byte for byte."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_EXEC = 7
GEOM = [(64, 64), (176, 144), (96, 80), (128, 96), (176, 144), (80, 64)]  # one stream each
FRAMES = (7, 6)  # pictures per stream of the two batches


def _kw(batch, i, **over):
    w, h = GEOM[i]
    kw = dict(width=w, height=h, frames=FRAMES[batch], idr_period=0, profile_idc=77, cabac=1, qp=28 + 2 * i, num_ref_frames=1 + i % 2,
              sub8x8_permille=200 * (i % 3), intra_in_p_permille=100 * (i % 2), seed=7100 + 10 * batch + i)
    kw.update(over)
    return kw


@pytest.fixture(scope="module")
def batches(sg, oracle_mod):
    """Two batches of six I/P CABAC streams, and what the oracle makes of them: per batch the cropped frames, stream-major, as K6 packs them."""
    out = []
    for b in range(2):
        streams = [sg.encode(**_kw(b, i))[0] for i in range(len(GEOM))]
        want = np.concatenate([oracle_mod.decode(s, crop=True)[0].reshape(-1) for s in streams])
        want.setflags(write=False)
        out.append((streams, want))
    return out


@pytest.fixture(scope="module")
def hooks(H):
    return H.load_hooks()  # (declares the signatures of the pass-group entries)


def _decoder(H, hooks, G, **kw):
    dec = H.Decoder(max_streams=len(GEOM), max_width=176, max_height=144, max_frames_per_batch=max(FRAMES), max_slices_per_frame=1, **kw)
    assert hooks.h264mi_internal_set_pass_group(dec._h, G) == 0
    return dec


def _waits(hooks, dec):
    p, g = ctypes.c_int64(-2), ctypes.c_int64(-2)
    assert hooks.h264mi_internal_pass_waits(dec._h, ctypes.byref(p), ctypes.byref(g)) == 0
    return p.value, g.value


def _gate_of(G, k, first_pass=0):
    """The gate of the k-th pass of an uninterrupted sequence of grouped passes that began at pass counter first_pass behind pass first_pass - 1."""
    if not G:
        return -1
    first = k - k % G
    return first_pass + first - 1 if first_pass + first > 0 else -1


def _run(H, hooks, batches, G, pack_every=False, side=False):
    """execute, prepare, execute ... N_EXEC times without a sync; K6 packs of (at least) the last two passes launched behind their executes.
    Returns the packs of the last two passes, the side information of every pass read (or []), and the statuses."""
    import torch
    dec = _decoder(H, hooks, G)
    try:
        packs, sides = {}, []
        dec.prepare(batches[0][0])
        for k in range(N_EXEC):
            b = k % 2
            dec.execute()
            assert _waits(hooks, dec) == (k, _gate_of(G, k)), (G, k)
            if pack_every or k >= N_EXEC - 2:
                n = batches[b][1].size
                packs[k] = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                assert dec.pack_batch(packs[k].data_ptr(), n) == n
            if side:
                t = torch.zeros(2 << 20, dtype=torch.uint8, device="cuda")
                n = dec.side_batch(t.data_ptr(), t.numel(), H.SIDE_NAMES)
                assert 0 < n <= t.numel()
                sides.append(t[:n])
            if k + 1 < N_EXEC:
                dec.prepare(batches[(k + 1) % 2][0])
        dec.sync()
        status = [dec.stream_status(i) for i in range(len(GEOM))]
        last = dec.read_frames  # the frames of the last pass through the host accessor as well
        tail = np.concatenate([last(i, crop=True, size=GEOM[i][0] * GEOM[i][1] * 3 // 2).reshape(-1) for i in range(len(GEOM))])
        host = {k: v.cpu().numpy() for k, v in packs.items()}
        return host, [s.cpu().numpy() for s in sides], status, tail
    finally:
        dec.close()


@pytest.fixture(scope="module")
def ungrouped(H, hooks, batches):
    return _run(H, hooks, batches, 0, pack_every=True, side=True)


def _check(batches, got, want_run, G):
    packs, sides, status, tail = got
    packs0, sides0, status0, tail0 = want_run
    assert status == [0] * len(GEOM) and status0 == [0] * len(GEOM)
    for k in sorted(packs):
        want = batches[k % 2][1]
        assert (packs[k][want.size:] == 0xA5).all()
        assert np.array_equal(packs[k][:want.size], want), "G = %d: pass %d differs from the oracle" % (G, k)
        assert np.array_equal(packs[k], packs0[k]), "G = %d: pass %d differs from the ungrouped run" % (G, k)
    assert set(packs) >= {N_EXEC - 2, N_EXEC - 1}
    assert np.array_equal(tail, batches[(N_EXEC - 1) % 2][1]) and np.array_equal(tail, tail0)
    for k, s in enumerate(sides):
        assert np.array_equal(s, sides0[k]), "G = %d: side information of pass %d differs from the ungrouped run" % (G, k)


def test_the_ungrouped_run_is_the_oracle(batches, ungrouped):
    _check(batches, ungrouped, ungrouped, 0)
    assert len(ungrouped[1]) == N_EXEC


@pytest.mark.parametrize("G", [2, 3])
def test_seven_executes_one_sync(H, hooks, batches, ungrouped, G):
    _check(batches, _run(H, hooks, batches, G), ungrouped, G)


@pytest.mark.parametrize("G", [2, 3])
def test_with_pack_and_side_reads_between_passes(H, hooks, batches, ungrouped, G):
    """K6 after every pass (last_pack: the next reconstruction waits for it) and K11 after every pass (last_side: the next entropy stream waits for it)."""
    got = _run(H, hooks, batches, G, pack_every=True, side=True)
    assert len(got[0]) == N_EXEC and len(got[1]) == N_EXEC
    _check(batches, got, ungrouped, G)


@pytest.mark.parametrize("G", [2, 3])
def test_an_exclusive_pass_in_mid_sequence(H, hooks, sg, oracle_mod, batches, G):
    """A pool of one residual block per macroblock: 45 chunks of 2048 blocks for this geometry.  The light batches take a chunk per slice (42, 36); the
    hungry one -- QP 1 on loud noise, every block of every macroblock coded, 99 macroblocks x 26 blocks a picture -- takes two per slice, runs out
    (status 40), and h264mi_batch_sync repeats it alone with the three pools as one (135 chunks).  That pass closes the open group; the group after it is
    gated on it.
    What this does and does not show: with G = 2 the repeated pass arrives when the decoder's first, gateless group (passes 0 and 1) is already full, so
    only the G = 3 case would fail if an exclusive pass did not close an open group.  And h264mi_internal_pass_waits reports the decision taken next to
    the wait, not the wait itself: the gate only adds ordering, so these small batches decode the same bytes with or without it.  The tests here pin the
    bookkeeping and that nothing breaks; that the wait acts is what the kernel trace of the bench shows (profiles/pass_groups.txt).  The event graph is
    modelled in tests/test_pass_groups.py."""
    import torch
    hungry = [sg.encode(**_kw(0, i, width=176, height=144, qp=1, noise=100, sub8x8_permille=0, intra_in_p_permille=0, seed=7300 + i))[0] for i in range(len(GEOM))]
    want_hungry = np.concatenate([oracle_mod.decode(s, crop=True)[0].reshape(-1) for s in hungry])
    runs = {}
    for g in (0, G):
        dec = _decoder(H, hooks, g, coef_blocks_per_mb=1, max_bitstream_bytes=int(1.1 * sum(len(s) for s in hungry)) + (1 << 20))
        try:
            dec.prepare(batches[1][0])
            dec.execute()
            assert _waits(hooks, dec) == (0, -1)
            dec.prepare(hungry)
            dec.execute()
            assert _waits(hooks, dec) == (1, -1)  # (grouped: the decoder's first group has no gate)
            dec.sync()  # ... finds the exhaustion and repeats pass 1 exclusively: record set 0, i.e. pass counter 3
            used, cap = dec.coef_pool()
            assert used > cap, (used, cap)
            assert _waits(hooks, dec) == (3, -1), "an exclusive pass waits for no gate"
            assert [dec.stream_status(i) for i in range(len(GEOM))] == [0] * len(GEOM)
            mid = torch.zeros(want_hungry.size, dtype=torch.uint8, device="cuda")
            assert dec.pack_batch(mid.data_ptr(), mid.numel()) == mid.numel()
            packs = {}
            for k in range(N_EXEC - 2):  # five more passes, light batches alternately: pass counters 4 .. 8
                b = k % 2
                dec.prepare(batches[b][0])
                dec.execute()
                assert _waits(hooks, dec) == (4 + k, _gate_of(g, k, first_pass=4)), (g, k)
                if k >= N_EXEC - 4:
                    packs[k] = torch.zeros(batches[b][1].size, dtype=torch.uint8, device="cuda")
                    assert dec.pack_batch(packs[k].data_ptr(), packs[k].numel()) == packs[k].numel()
            dec.sync()
            used, cap = dec.coef_pool()
            assert [dec.stream_status(i) for i in range(len(GEOM))] == [0] * len(GEOM)
            assert np.array_equal(mid.cpu().numpy(), want_hungry), "the repeated pass"
            runs[g] = {k: v.cpu().numpy() for k, v in packs.items()}
            for k, v in runs[g].items():
                assert np.array_equal(v, batches[k % 2][1]), (g, k)
        finally:
            dec.close()
    assert sorted(runs[G]) == sorted(runs[0]) == [N_EXEC - 4, N_EXEC - 3]
    for k in runs[G]:
        assert np.array_equal(runs[G][k], runs[0][k])


def test_a_batch_with_b_slices_stays_ungrouped(H, hooks, sg, oracle_mod):
    """I B B P: the plan refuses it, and forcing a group size changes nothing -- no pass waits for a gate, the frames are the oracle's."""
    assert H.load_hooks().h264mi_internal_pass_group_plan(100000, 6144, 256, 1) == 0
    kws = [dict(width=176, height=144, frames=7, idr_period=0, profile_idc=77, cabac=1, bframes=2, num_ref_frames=3, seed=7400 + i) for i in range(4)]
    streams = [sg.encode(**kw)[0] for kw in kws]
    want = [oracle_mod.decode(s, crop=True)[0] for s in streams]
    got = {}
    for G in (0, 3):
        dec = H.Decoder(max_streams=4, max_width=176, max_height=144, max_frames_per_batch=7, max_slices_per_frame=1)
        try:
            assert hooks.h264mi_internal_set_pass_group(dec._h, G) == 0
            dec.prepare(streams)
            for k in range(N_EXEC):
                dec.execute()
                assert _waits(hooks, dec) == (k, -1)
            dec.sync()
            got[G] = [dec.read_frames(i, crop=True, size=176 * 144 * 3 // 2) for i in range(4)]
            assert [dec.stream_status(i) for i in range(4)] == [0] * 4
        finally:
            dec.close()
    for i in range(4):
        assert np.array_equal(got[3][i], want[i]) and np.array_equal(got[0][i], want[i]), i


def test_profiling_between_groups(H, hooks, batches, ungrouped):
    """set_profiling(True) between groups: the serialised pass waits for no gate and closes the group, its kernel times are reported, the group after it is
    gated on it, and the frames are what they were."""
    import torch
    G = 2
    dec = _decoder(H, hooks, G)
    try:
        dec.prepare(batches[0][0])
        for k in range(3):
            dec.execute()
            assert _waits(hooks, dec) == (k, _gate_of(G, k))
        dec.set_profiling(True)
        dec.execute()
        assert _waits(hooks, dec) == (3, -1)
        dec.sync()
        t = dec.kernel_times_ms()
        assert t["entropy"] > 0 and t["deblock"] > 0 and t["total"] >= t["entropy"]
        dec.set_profiling(False)
        packs = {}
        for k in range(3):
            dec.prepare(batches[k % 2][0])
            dec.execute()
            assert _waits(hooks, dec) == (4 + k, _gate_of(G, k, first_pass=4))
            packs[k] = torch.zeros(batches[k % 2][1].size, dtype=torch.uint8, device="cuda")
            assert dec.pack_batch(packs[k].data_ptr(), packs[k].numel()) == packs[k].numel()
        dec.sync()
        for k in range(3):
            assert np.array_equal(packs[k].cpu().numpy(), batches[k % 2][1]), k
        assert [dec.stream_status(i) for i in range(len(GEOM))] == [0] * len(GEOM)
    finally:
        dec.close()
