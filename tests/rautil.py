"""Random access (h264mi_decoder_set_random_access): the open-GOP recipes of the generator, where their entry points are, and the streams cut there.
Shared by the CPU tests (test_random_access_host.py, test_random_access_streams.py) and the GPU tests (test_random_access_gpu.py)."""
import functools

# Every recipe: only the first picture is an IDR picture, a non-IDR I anchor with a recovery point every 6 frames (rounded up to the anchor distance).
# 176x144 as far as the generator can: field pictures need an even number of macroblock rows, so (d) and (e) are 176x128.
BASE = dict(width=176, height=144, frames=24, idr_period=0, open_gop_period=6, qp=30)
RECIPES = {
    "a": dict(BASE, profile_idc=66, cabac=0, bframes=0, num_ref_frames=3, seed=701),
    "b": dict(BASE, profile_idc=77, cabac=1, bframes=2, num_ref_frames=2, bskip_permille=200, seed=702),
    "c": dict(BASE, profile_idc=100, cabac=1, transform8x8=1, bframes=3, b_pyramid=1, bskip_permille=200, seed=703),
    "d": dict(BASE, height=128, frames=14, profile_idc=77, cabac=0, field_pics=1, bframes=0, num_ref_frames=2, seed=704),
    "e": dict(BASE, height=128, frames=14, profile_idc=77, cabac=0, field_pics=2, bframes=2, num_ref_frames=2, seed=705),
    "f": dict(BASE, profile_idc=66, cabac=0, bframes=0, num_ref_frames=3, poc_type=1, seed=706),
}


def nal_units(stream):
    """[(start, end, nal_unit_type)] of an Annex-B stream; `start` is the first byte of the unit's start code (its leading zero byte included)."""
    starts, i, n = [], 0, len(stream)
    while i + 3 <= n:
        if stream[i] == 0 and stream[i + 1] == 0 and stream[i + 2] == 1:
            starts.append((i - 1 if i > 0 and stream[i - 1] == 0 else i, i + 3))
            i += 3
        else:
            i += 1
    ends = [s for s, _ in starts[1:]] + [n]
    return [(s, e, stream[h] & 31) for (s, h), e in zip(starts, ends)]


def access_unit_starts(stream):
    """Byte offsets at which the access units of a generator stream begin: the first NAL unit of every run of non-slice units, or a slice whose
    first_mb_in_slice is 0 (ue: the first payload bit is 1) right behind another slice."""
    units, out, prev_slice = nal_units(stream), [], True
    for s, e, t in units:
        h = s + (4 if stream[s:s + 4] == b"\x00\x00\x00\x01" else 3)
        is_slice = t in (1, 5)
        if (not is_slice and prev_slice) or (is_slice and prev_slice and stream[h + 1] & 0x80):
            out.append(s)
        prev_slice = is_slice
    return out


class Case:
    """One recipe: stream, reconstruction (coding order), the generator's entry points and what a decoder that joins at each of them must deliver."""

    def __init__(self, sg, name):
        self.name, self.kw = name, RECIPES[name]
        self.stream, self.recon, _ = sg.encode(**self.kw)
        self.gen_entries = sg.last_entries()  # (frame in coding order, leading pictures)
        self.features = sg.last_features()
        self.units = nal_units(self.stream)
        self.pics_per_frame = 2 if self.kw.get("field_pics") else 1
        self.frames = self.kw["frames"]
        self.w, self.h = self.kw["width"], self.kw["height"]
        # the SPS units behind the first one: each starts the access unit of an entry picture
        sps = [i for i, (_, _, t) in enumerate(self.units) if t == 7]
        assert len(sps) == 1 + len(self.gen_entries), (sps, self.gen_entries)
        self.entries = []
        for ui, (t, lead) in zip(sps[1:], self.gen_entries):
            slices = [i for i in range(ui) if self.units[i][2] in (1, 5)]
            g = slices[-3]  # a slice a few units in front: the garbage cut lands in its middle
            self.entries.append(dict(unit=ui, cut=self.units[ui][0], garbage_cut=(self.units[g][0] + self.units[g][1]) // 2, frame=t, leading=lead,
                                     expect=[t] + list(range(t + 1 + lead // self.pics_per_frame, self.frames))))


@functools.lru_cache(maxsize=None)
def _case(name):
    import streamgen
    return Case(streamgen, name)


def case(sg, name):
    return _case(name)
