"""Error concealment of field pictures (h264mi_config.conceal_errors with H264MI_CONCEAL_FIELDS): lost and damaged slices of non-IDR field pictures
are reconstructed as a zero-motion copy of entry 0 of the field's initial P list (8.2.4.2.5).  The yardstick is the oracle's decode of the REPAIRED
stream (tests/concealutil2.py: make_fields); every GPU comparison is bit-exact."""
import os

import numpy as np
import pytest

import concealutil as cu
import concealutil2 as c2
import hostprog
from concealutil2 import FIELD_CASES
from conftest import pictures_of

SLICES, FIELDS = 1, 4  # H264MI_CONCEAL_SLICES, H264MI_CONCEAL_FIELDS
MODES = ("lost", "damaged", "header")


# ---------------------------------------------------------------- CPU: the writer and the rule
def test_the_matrix_has_the_required_shapes():
    kws = list(FIELD_CASES.values())
    assert len(kws) >= 8
    assert {kw["cabac"] for kw in kws} == {0, 1} and {kw["field_pics"] for kw in kws} == {1, 2}
    assert any(kw.get("bframes") for kw in kws) and any(not kw.get("bframes") for kw in kws)
    assert {kw.get("num_ref_frames", 1) for kw in kws} >= {1, 2, 3}
    assert any(kw.get("weighted_pred") for kw in kws)
    assert {kw.get("deblock_idc", 0) for kw in kws} == {0, 1, 2}
    assert all(kw["slices"] == 3 and kw["width"] >= 176 and kw["height"] >= 128 and kw["idr_period"] == 0 for kw in kws)


@pytest.mark.parametrize("name", sorted(FIELD_CASES))
def test_repaired_field_stream_is_a_valid_stream(name, sg, oracle_mod):
    """The oracle decodes the repaired stream with the frame count and PicOrderCnt list of the original, in every mode; the damage meets the
    conditions of the matrix (concealutil2.check_field_picks: the second field of the IDR frame, first / middle / last / adjacent slices, both
    parities, P and -- where the recipe has them -- B fields); frames before the first damaged one are untouched."""
    kw = FIELD_CASES[name]
    stream, rec, _ = sg.encode(**kw)
    ref, info = oracle_mod.decode(stream, crop=False)
    pocs = list(oracle_mod.last_pocs)
    _, _, pics = cu.parse(stream)
    assert all(p[0].hdr.field_pic for p in pics) and len(pics) == 2 * kw["frames"]
    if kw.get("bframes"):
        assert any(pics[p][0].hdr.slice_type % 5 == 1 for p, _ in c2.field_picks(pics)), "a slice of a B field"
    for mode in MODES:
        damaged, repaired, per_frame, n = c2.make_fields(stream, mode=mode)
        assert damaged != stream and repaired != stream and n >= 5
        out, info2 = oracle_mod.decode(repaired, crop=False)
        assert info2.n_frames == info.n_frames == kw["frames"]
        assert list(oracle_mod.last_pocs) == pocs
        first = min(f for f, c in enumerate(per_frame) if c)
        assert np.array_equal(out[:first], ref[:first])
        assert not np.array_equal(out[first], ref[first])


def test_second_field_of_the_idr_frame_is_copied_from_its_first_field(sg, oracle_mod):
    """deblock_idc 1: the intact slices filter nothing, the replaced slice (a whole macroblock row of the second field of the IDR frame) filters its own
    top edge only.  Below the three filtered rows its macroblocks equal the rows of the OTHER parity of the same frame: entry 0 of the field list of
    a second field is the first field of its frame."""
    kw = FIELD_CASES["field_bottom_first_refs3_idc1"]
    stream = sg.encode(**kw)[0]
    _, repaired, _, _ = c2.make_fields(stream)
    out, _ = oracle_mod.decode(repaired, crop=False)
    _, _, pics = cu.parse(stream)
    s = pics[1][1]
    assert pics[0][0].type == 5 and s.type == 1 and s.hdr.field_pic and s.hdr.frame_num == pics[0][0].hdr.frame_num
    W, Hh = s.wmb * 16, s.hmb * 32
    luma = out[0][:W * Hh].reshape(Hh, W)
    par = int(s.hdr.bottom_field)
    mine, other = luma[par::2], luma[1 - par::2]
    assert len(s.mbs) == s.wmb
    for a in s.mbs:
        x, y = a % s.wmb, a // s.wmb
        assert np.array_equal(mine[16 * y + 3:16 * y + 16, 16 * x:16 * x + 16], other[16 * y + 3:16 * y + 16, 16 * x:16 * x + 16]), a
    assert not np.array_equal(mine, other)


@pytest.fixture(scope="module")
def host_pocs(tmp_path_factory):
    import shutil
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("host_pocs_fields")
    return hostprog.build("host_pocs.sh", tmp), tmp


@pytest.mark.parametrize("name", sorted(FIELD_CASES))
def test_host_tolerates_unparsable_headers_in_concealable_fields(name, host_pocs, sg, oracle_mod):
    """Picture management alone (no GPU): with value 5 a type-1 slice whose header does not parse is a lost slice of a field picture -- the second
    field of the IDR frame included -- and the PicOrderCnt list is the oracle's for the repaired stream; with value 1 the stream is refused."""
    import subprocess
    prog, tmp = host_pocs
    kw = FIELD_CASES[name]
    damaged, repaired, _, _ = c2.make_fields(sg.encode(want_recon=False, **kw)[0], mode="header")
    oracle_mod.decode(repaired, crop=False)
    pocs = [int(x) for x in oracle_mod.last_pocs]
    path = os.path.join(str(tmp), "f.h264")
    open(path, "wb").write(damaged)
    W, Hc = (kw["width"] + 15) & ~15, (kw["height"] + 15) & ~15
    for v in (SLICES, SLICES | FIELDS):
        r = subprocess.run([prog, path, str(W), str(Hc), str(pictures_of(kw)), "8", str(v), str(kw["cabac"])], capture_output=True, text=True, timeout=120)
        if v == SLICES:
            assert r.returncode == 1 and "stream status -2" in r.stderr
        else:
            assert r.returncode == 0, r.stderr[-1000:]
            assert [int(line.split()[0]) for line in r.stdout.splitlines() if line.strip() and not line.startswith("order")] == pocs


# ---------------------------------------------------------------- GPU
class _x_wgs:
    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.old = os.environ.get("H264MI_X_WGS")
        if self.n is not None:
            os.environ["H264MI_X_WGS"] = str(self.n)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("H264MI_X_WGS", None)
        else:
            os.environ["H264MI_X_WGS"] = self.old


def _decoder(H, kw, streams, **cfg):
    W, Hc = (kw["width"] + 15) // 16 * 16, (kw["height"] + 15) // 16 * 16
    return H.Decoder(max_streams=len(streams), max_width=W, max_height=Hc, max_frames_per_batch=pictures_of(kw), max_slices_per_frame=max(cu.nslices(kw), 1),
                     max_bitstream_bytes=sum(len(s) for s in streams) * 2 + (1 << 20), allow_unpinned_field_cabac=int(bool(kw["cabac"])), **cfg)


def _check_concealed(H, oracle_mod, kw, stream, mode):
    damaged, repaired, per_frame, n_slices = c2.make_fields(stream, mode=mode)
    want, _ = oracle_mod.decode(repaired, crop=False)
    want_pocs = list(oracle_mod.last_pocs)
    for x in (None, 0, 512):
        with _x_wgs(x):
            dec = _decoder(H, kw, [damaged], conceal_errors=SLICES | FIELDS)
            try:
                dec.decode([damaged])
                if mode == "damaged":  # precondition: the entropy kernels reported every damaged slice (otherwise the DAMAGE is at fault, not the feature)
                    assert dec.concealed()[0] == n_slices, "damage not detected: %r" % (dec.concealed(),)
                assert dec.stream_status(0) == 0
                assert dec.frame_count(0) == kw["frames"]
                out = dec.read_frames(0, crop=False)
                bad = [i for i in range(len(want)) if not np.array_equal(out[i], want[i])]
                assert not bad, "frames %r differ from the oracle's decode of the repaired stream (H264MI_X_WGS=%r)" % (bad, x)
                assert [dec.frame_info(0, f).pic_order_cnt for f in range(kw["frames"])] == want_pocs
                assert [dec.frame_concealed(0, f) for f in range(kw["frames"])] == per_frame
                assert dec.concealed() == (0 if mode == "lost" else n_slices, sum(per_frame))
                assert dec.concealed_pictures() == 0
                assert dec.unpinned_failures() == (n_slices if mode == "damaged" and kw["cabac"] else 0)  # counted as before, concealed or not
            finally:
                dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(FIELD_CASES))
def test_gpu_field_slices_are_concealed(name, mode, H, sg, oracle_mod):
    kw = FIELD_CASES[name]
    _check_concealed(H, oracle_mod, kw, sg.encode(**kw)[0], mode)


@pytest.mark.gpu
def test_gpu_without_the_bit_field_pictures_stay_as_they_are(H, sg):
    """Values 0, 1 and 3 on a damaged field slice: one error, one status, nothing concealed."""
    kw = FIELD_CASES["field_cavlc_refs2_idc2"]
    stream = sg.encode(**kw)[0]
    res = []
    for mode, want in (("damaged", -8), ("header", -2)):
        damaged = c2.make_fields(stream, mode=mode)[0]
        for v in (0, 1, 3):
            dec = _decoder(H, kw, [damaged], conceal_errors=v)
            try:
                code = 0
                try:
                    dec.decode([damaged])
                except H.H264MIError as e:
                    code = e.code
                res.append((code, dec.stream_status(0), dec.concealed()))
                assert res[-1] == (want, want, (0, 0)), (mode, v, res[-1])
            finally:
                dec.close()
