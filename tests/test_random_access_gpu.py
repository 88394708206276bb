"""Random access on the device: a stream joined at a recovery point (h264mi_decoder_set_random_access) must give, byte for byte, the generator's
reconstruction of exactly the pictures from the entry picture on, minus the leading ones -- decoded alone, beside an ordinary stream, after an error,
after a reset, through BatchServer and through the C example.  The streams are tests/rautil.py's; picture management alone is held to the whole
stream on the CPU (tests/test_random_access_host.py)."""
import os
import subprocess

import numpy as np
import pytest

import rautil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NAMES = sorted(rautil.RECIPES)


def _decoder(H, streams=1, frames=64, **kw):
    return H.Decoder(max_streams=streams, max_width=176, max_height=144, max_frames_per_batch=frames, max_slices_per_frame=8, **kw)


@pytest.mark.parametrize("name", NAMES)
def test_gpu_join_at_every_entry_point(H, sg, name):
    c = rautil.case(sg, name)
    dec = _decoder(H)
    try:
        with pytest.raises(H.H264MIError):  # the mode is off: a stream that does not begin with an IDR picture is refused, as ever
            dec.decode([c.stream[c.entries[0]["cut"]:]])
        dec.set_random_access(True)
        for k, en in enumerate(c.entries):
            for kind in ("cut", "garbage_cut"):
                dec.reset_stream(0)
                dec.decode([c.stream[en[kind]:]])
                assert dec.stream_status(0) == 0
                assert np.array_equal(dec.read_frames(0, crop=False), c.recon[en["expect"]]), (k, kind)
                fe = [dec.frame_entry(0, f) for f in range(dec.frame_count(0))]
                assert [e.entry for e in fe] == [1] + [0] * (len(fe) - 1) and fe[0].recovery_point == 1 and fe[0].exact_match_flag == 1
                assert dec.frame_info(0, 0).new_sequence == 1 and dec.frame_info(0, 0).idr == 0
                ra = dec.random_access_stats(0)
                assert ra[0] == 1 and ra[2] == en["leading"] and (ra[1] > 0) == (kind == "garbage_cut")
        dec.reset_stream(0)
        dec.decode([c.stream])  # the whole stream with the mode on
        assert np.array_equal(dec.read_frames(0, crop=False), c.recon) and dec.random_access_stats(0) == (0, 0, 0)
    finally:
        dec.close()


def _gop_chunks(c):
    """The stream cut in front of every entry point's access unit"""
    cuts = [0] + [en["cut"] for en in c.entries] + [len(c.stream)]
    return [c.stream[a:b] for a, b in zip(cuts, cuts[1:])]


@pytest.mark.parametrize("mode", [True, False])
def test_gpu_resume_after_an_error(H, sg, mode):
    """Recipe (b), isolation, no concealment: the slice data of the first P picture is replaced by 01 bytes, the stream is fed one group of pictures
    per batch.  The damaged batch reports H264MI_EDECODE; with the mode on the stream comes back at the next recovery point, with it off it stays out."""
    c = rautil.case(sg, "b")
    nals = H.read_nal_units(c.stream)
    offs = [n.Offset - 4 for n in nals] + [len(c.stream)]
    k = [i for i, n in enumerate(nals) if n.Type in (1, 5)][1]  # coding order I P B B: the P picture
    sps = H.NewSPS(nals[0].RBSP())
    hdr = H.NewSliceContext(H.VideoStream(sps, H.NewPPS(sps, nals[1].RBSP())), nals[k], nals[k].RBSP()).Slice.Header
    assert hdr.slice_type % 5 == 0
    keep = 4 + 1 + (hdr.slice_data_bit_offset + 7) // 8  # start code, NAL header byte, every byte the slice header has bits in
    chunks = _gop_chunks(c)
    chunks[0] = c.stream[:offs[k] + keep] + b"\x01" * 24 + c.stream[offs[k + 1]:len(chunks[0])]
    dec = _decoder(H)
    try:
        dec.set_isolation(True)
        dec.set_random_access(mode)
        dec.decode([chunks[0]])
        assert dec.stream_status(0) == -8
        first, lead = c.entries[0]["frame"], c.entries[0]["leading"]
        bounds = [en["frame"] for en in c.entries] + [c.frames]
        for i, ch in enumerate(chunks[1:]):
            dec.decode([ch])
            assert dec.stream_status(0) == 0
            if not mode:  # today's behaviour: nothing before the next IDR picture, and there is none
                assert dec.frame_count(0) == 0
                continue
            want = [first] + list(range(first + 1 + lead, bounds[1])) if i == 0 else list(range(bounds[i], bounds[i + 1]))
            assert np.array_equal(dec.read_frames(0, crop=False), c.recon[want]), i
        assert dec.random_access_stats(0)[0] == (1 if mode else 0)
    finally:
        dec.close()


def test_gpu_joining_stream_beside_an_ordinary_one(H, sg):
    a, b = rautil.case(sg, "a"), rautil.case(sg, "c")
    en = b.entries[0]
    dec = _decoder(H, streams=2)
    try:
        dec.set_random_access(True)
        dec.decode([a.stream, b.stream[en["garbage_cut"]:]])
        assert dec.stream_status(0) == 0 and dec.stream_status(1) == 0
        assert np.array_equal(dec.read_frames(0, crop=False), a.recon), "the ordinary stream's frames are unchanged"
        assert np.array_equal(dec.read_frames(1, crop=False), b.recon[en["expect"]])
        assert dec.random_access_stats(0) == (0, 0, 0) and dec.random_access_stats(1)[0] == 1
    finally:
        dec.close()


class _Conn:
    """A connection that delivers `data` in pieces and then closes"""

    def __init__(self, data, piece=1500):
        self.data, self.at, self.piece = data, 0, piece

    def recv(self, n):
        out = self.data[self.at:self.at + min(n, self.piece)]
        self.at += len(out)
        return out


def test_gpu_batch_server_client_that_starts_in_the_middle(H, sg):
    c = rautil.case(sg, "b")
    en = c.entries[1]
    got = []
    bs = H.BatchServer(max_connections=1, max_width=176, max_height=144, frames_per_batch=5, random_access=True, on_frames=lambda i, f: got.append(f))
    assert bs.add(_Conn(c.stream[en["garbage_cut"]:])) == 0
    for _ in range(10000):
        if not bs.active():
            break
        bs.tick()
    assert not bs.active() and bs.errors[0] == 0
    assert np.array_equal(np.concatenate(got), c.recon[en["expect"]])
    bs.decoder.close()


def test_gpu_c_example_random_access(sg, tmp_path):
    c = rautil.case(sg, "c")
    en = c.entries[0]
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    src, dst = tmp_path / "in.h264", tmp_path / "out.yuv"
    src.write_bytes(c.stream[en["cut"]:])
    prog = os.path.join(ROOT, "examples", "h264mi_decode")
    subprocess.run([prog, str(src), str(dst), "6", "--random-access"], stderr=subprocess.PIPE, check=True, timeout=120)
    assert np.array_equal(np.frombuffer(dst.read_bytes(), dtype=np.uint8), c.recon[en["expect"]].ravel())
    assert subprocess.run([prog, str(src), str(dst), "6"], stderr=subprocess.PIPE, timeout=120).returncode != 0, "without the flag the cut file is refused"


def test_gpu_seek_after_decoder_reset(H, sg):
    """h264mi_decoder_reset is "seek": feeding from an entry point afterwards decodes from it with the mode on (parameter sets are kept, the counters too)"""
    c = rautil.case(sg, "e")
    en = c.entries[1]
    dec = _decoder(H)
    try:
        dec.set_random_access(True)
        dec.decode([c.stream[:c.entries[0]["cut"]]])
        assert np.array_equal(dec.read_frames(0, crop=False), c.recon[:c.entries[0]["frame"]])
        dec.reset()
        dec.decode([c.stream[en["cut"]:]])
        assert np.array_equal(dec.read_frames(0, crop=False), c.recon[en["expect"]])
        assert dec.frame_entry(0, 0).entry == 1 and dec.random_access_stats(0) == (1, 0, en["leading"])
    finally:
        dec.close()
