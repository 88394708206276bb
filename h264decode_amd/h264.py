"""Host-side mirror of the reference's Go package `h264` (same names, argument meaning and -- where
the reference is right -- values), implemented on the C ABI of libh264mi.so.

Reference            -> here
  NalUnit            h264/nalUnit.go:3-30      -> NalUnit (fields in CamelCase as in Go)
  NewNalUnit         h264/nalUnit.go:75        -> NewNalUnit(frame, numBytesInNal)
  (*NalUnit).RBSP    h264/nalUnit.go:72        -> NalUnit.RBSP()
  SPS / NewSPS       h264/sps.go:9,192         -> SPS / NewSPS(rbsp, showPacket)
  PPS / NewPPS       h264/pps.go:10,40         -> PPS / NewPPS(sps, rbsp, showPacket)
  SliceHeader        h264/slice.go:23          -> SliceHeader
  SliceContext       h264/slice.go:13          -> SliceContext (NalUnit, SPS, PPS, Slice.Header)
  NewSliceContext    h264/slice.go:835         -> NewSliceContext(videoStream, nalUnit, rbsp, showPacket)
  VideoStream        h264/slice.go:8           -> VideoStream(SPS, PPS, Slices)
  readNalUnit loop   h264/server.go:64-166     -> read_nal_units(bytes)
New (the reference has no pixel type): Decoder -- batched GPU decode to Y/Cb/Cr planes.

Error behaviour: the reference panics / os.Exit()s on malformed input (h264/server.go:136-143); here
every failure raises H264MIError carrying the C status code."""
import builtins
import ctypes

import numpy as np

from . import _lib
from ._lib import H264MIError, check

NALU_TYPE_NAMES = {  # h264/frame.go:28-60
    0: "unspecified", 1: "coded slice of non-IDR picture", 2: "coded slice data partition A", 3: "coded slice data partition B",
    4: "coded slice data partition C", 5: "coded slice of an IDR picture", 6: "SEI", 7: "SPS", 8: "PPS", 9: "AUD",
    10: "end of sequence", 11: "end of stream", 12: "filler data", 13: "SPS extension", 14: "prefix NAL unit",
    15: "subset SPS", 19: "auxiliary slice", 20: "slice extension", 21: "slice extension for depth view"}


def _camel(name):
    return "".join(p.capitalize() if not p.isdigit() else p for p in name.split("_"))


class _Mirror:
    """Exposes the fields of a C struct under the reference's CamelCase names (and snake_case)."""
    _c = None

    def __getattr__(self, name):
        c = object.__getattribute__(self, "_c")
        for fname, _ in c._fields_:
            if name == fname or name == _camel(fname):
                v = getattr(c, fname)
                if hasattr(v, "_length_"):
                    return np.ctypeslib.as_array(v).copy()
                return v
        raise AttributeError(name)

    def as_dict(self):
        out = {}
        for fname, _ in self._c._fields_:
            v = getattr(self._c, fname)
            out[fname] = np.ctypeslib.as_array(v).tolist() if hasattr(v, "_length_") else v
        return out


class NalUnit(_Mirror):
    def __init__(self, c, rbsp):
        self._c, self._rbsp = c, rbsp

    def RBSP(self):
        return self._rbsp

    # Go field names that differ from the C struct's snake_case conversion
    NumBytes = property(lambda s: s._c.num_bytes)
    RefIdc = property(lambda s: s._c.ref_idc)
    Type = property(lambda s: s._c.type)


class SPS(_Mirror):
    def __init__(self, c):
        self._c = c

    ID = property(lambda s: s._c.id)  # h264/sps.go:12


class PPS(_Mirror):
    def __init__(self, c, slice_group_id=None):
        self._c = c
        self._ids = slice_group_id if slice_group_id is not None else np.zeros(0, dtype=np.uint8)

    SPSID = property(lambda s: s._c.sps_id)
    ID = property(lambda s: s._c.id)
    SliceGroupChangeDirection = property(lambda s: bool(s._c.slice_group_change_direction))
    SliceGroupId = property(lambda s: s._ids.copy())  # h264/pps.go:23 (slice_group_map_type 6: one entry per map unit)


class SliceHeader(_Mirror):
    def __init__(self, c):
        self._c = c

    PPSID = property(lambda s: s._c.pps_id)
    SliceQPy = property(lambda s: s._c.slice_qp_y)


class Slice:
    def __init__(self, header):
        self.Header, self.Data = header, None  # slice_data() is decoded on the GPU (Decoder)


class SliceContext:
    def __init__(self, nal, sps, pps, header):
        self.NalUnit, self.SPS, self.PPS, self.Slice = nal, sps, pps, Slice(header)


class VideoStream:
    def __init__(self, sps=None, pps=None):
        self.SPS, self.PPS, self.Slices = sps, pps, []


def NewNalUnit(frame: bytes, numBytesInNal: int = None) -> NalUnit:
    n = len(frame) if numBytesInNal is None else numBytesInNal
    L = _lib.load()
    c = _lib.Nal()
    rbsp = (ctypes.c_uint8 * max(n, 1))()
    rl = ctypes.c_size_t(0)
    check(L.h264mi_nal_parse(frame, n, ctypes.byref(c), rbsp, ctypes.byref(rl)))
    return NalUnit(c, bytes(rbsp[:rl.value]))


def NewSPS(rbsp: bytes, showPacket: bool = False) -> SPS:
    c = _lib.Sps()
    check(_lib.load().h264mi_sps_parse(rbsp, len(rbsp), ctypes.byref(c)))
    return SPS(c)


def NewPPS(sps: SPS, rbsp: bytes, showPacket: bool = False) -> PPS:
    c = _lib.Pps()
    L = _lib.load()
    check(L.h264mi_pps_parse(ctypes.byref(sps._c), rbsp, len(rbsp), ctypes.byref(c)))
    ids = None
    if c.num_slice_groups_minus1 > 0 and c.slice_group_map_type == 6:
        ids = np.zeros(c.pic_size_in_map_units_minus1 + 1, dtype=np.uint8)
        n = ctypes.c_size_t(0)
        check(L.h264mi_pps_slice_group_ids(ctypes.byref(sps._c), rbsp, len(rbsp), ids.ctypes.data, ids.size, ctypes.byref(n)))
    return PPS(c, ids)


def _sg_args(pps, header):
    ids = pps._ids
    cycle = header.SliceGroupChangeCycle if header is not None else 0
    return (ids.ctypes.data if ids.size else None), ids.size, int(cycle)


def MapUnitToSliceGroupMap(sps: SPS, pps: PPS, header=None) -> np.ndarray:
    """mapUnitToSliceGroupMap, 8.2.2.1-8.2.2.7 (h264/slice.go:457-529; the reference implements types 0-2)."""
    out = np.zeros((sps.PicWidthInMbsMinus1 + 1) * (sps.PicHeightInMapUnitsMinus1 + 1), dtype=np.uint8)
    ids, n_ids, cycle = _sg_args(pps, header)
    check(_lib.load().h264mi_map_unit_to_slice_group_map(ctypes.byref(sps._c), ctypes.byref(pps._c), ids, n_ids, cycle, out.ctypes.data, out.size, None))
    return out


def MbToSliceGroupMap(sps: SPS, pps: PPS, header=None) -> np.ndarray:
    """mbToSliceGroupMap, 8.2.2.8 (h264/slice.go:134-158)."""
    field = bool(header.FieldPic) if header is not None else False
    n = (sps.PicWidthInMbsMinus1 + 1) * (sps.PicHeightInMapUnitsMinus1 + 1) * (1 if (sps.FrameMbsOnly or field) else 2)
    out = np.zeros(n, dtype=np.uint8)
    ids, n_ids, cycle = _sg_args(pps, header)
    check(_lib.load().h264mi_mb_to_slice_group_map(ctypes.byref(sps._c), ctypes.byref(pps._c), ids, n_ids, cycle, int(field), out.ctypes.data, out.size, None))
    return out


def nextMbAddress(n: int, sps: SPS, pps: PPS, header=None) -> int:
    """(8-17), h264/slice.go:530-552: the next macroblock of n's slice group; PicSizeInMbs when there is none."""
    m = MbToSliceGroupMap(sps, pps, header)
    return int(_lib.load().h264mi_next_mb_address(m.ctypes.data, m.size, n))


def NewSliceContext(videoStream: VideoStream, nalUnit: NalUnit, rbsp: bytes, showPacket: bool = False) -> SliceContext:
    c = _lib.SliceHdr()
    check(_lib.load().h264mi_slice_header_parse(ctypes.byref(videoStream.SPS._c), ctypes.byref(videoStream.PPS._c), nalUnit.RefIdc,
                                                nalUnit.Type, rbsp, len(rbsp), ctypes.byref(c)))
    return SliceContext(nalUnit, videoStream.SPS, videoStream.PPS, SliceHeader(c))


def read_nal_units(stream: bytes):
    """Annex-B scan: returns [NalUnit] (replaces the readNalUnit loop of h264/server.go:64-111,144-166)."""
    L = _lib.load()
    cap = 1024
    while True:
        arr = (_lib.Nal * cap)()
        n = ctypes.c_int32(0)
        r = L.h264mi_annexb_scan(stream, len(stream), arr, cap, ctypes.byref(n))
        if r == -7:
            cap *= 4
            continue
        check(r)
        break
    out = []
    for i in range(n.value):
        off, size = arr[i].offset, arr[i].num_bytes
        nu = NewNalUnit(stream[off:off + size], size)
        nu._c.offset = off
        out.append(nu)
    return out


CONCEAL_SLICES, CONCEAL_PICTURES, CONCEAL_FIELDS = 1, 2, 4  # bits of h264mi_config.conceal_errors (H264MI_CONCEAL_*): 2, 4 and 16 only together with CONCEAL_SLICES
CONCEAL_IDR = 16                         # H264MI_CONCEAL_IDR (bit 8 is unassigned)
CONCEAL_LONE_FIELDS = 64                 # H264MI_CONCEAL_LONE_FIELDS (only together with CONCEAL_SLICES | CONCEAL_FIELDS; bit 32 is unassigned)
CONCEAL_MAX_GAP = 16                     # H264MI_CONCEAL_MAX_GAP: the longest run of lost frames that is concealed
RA_OFF, RA_RECOVERY_POINT = 0, 1         # H264MI_RA_*: Decoder.set_random_access
FMT_I420, FMT_NV12, FMT_RGB24, FMT_RGBP = 0, 1, 2, 3  # H264MI_FMT_*: output formats of convert_frame / convert_batch / frames_tensor
CSC_AUTO, CSC_BT601, CSC_BT709 = 0, 1, 2              # H264MI_CSC_*: the matrix (AUTO: from each frame's own SPS) ...
CSC_FULL_RANGE, CSC_CHROMA_BILINEAR = 16, 32          # ... | full range (explicit matrix only) | bilinear chroma upsampling (default: nearest)
_FMT_NAMES = {"i420": FMT_I420, "nv12": FMT_NV12, "rgb24": FMT_RGB24, "rgbp": FMT_RGBP}
SCALE_BILINEAR, SCALE_AREA = 0, 1                     # H264MI_SCALE_*: filters of scale_frame / scale_batch / frames_tensor(size=...)
_FILTER_NAMES = {"bilinear": SCALE_BILINEAR, "area": SCALE_AREA}
DT_U8, DT_F16, DT_BF16, DT_F32 = 0, 1, 2, 3           # H264MI_DT_*: element types of tensor_batch / tensor_items / frames_tensor(dtype=...)
FIT_STRETCH, FIT_LETTERBOX = 0, 1                     # H264MI_FIT_*: how the picture is placed in the canvas
TENSOR_BGR = 1                                        # H264MI_TENSOR_BGR: colour c at channel position 2 - c
DEINT_FIELD, DEINT_BLEND, DEINT_EDGE = 0, 1, 2        # H264MI_DEINT_*: modes of Decoder.deinterlace / frames_tensor(deinterlace=...)
DEINT_PARITY_FIRST = -1                               # H264MI_DEINT_PARITY_FIRST: the frame's own first_parity (Decoder.frame_fields)
# H264MI_SIDE_*: planes of Decoder.side_batch / side_items / side_info, in the order they are written; SIDE_NAMES[i] is bit 1 << i
SIDE_NAMES = ("type", "qp", "nz", "slice", "mvx0", "mvy0", "ref0", "dpoc0", "mvx1", "mvy1", "ref1", "dpoc1")
SIDE_ALL = 0xFFF
MB_NONE, MB_I4x4, MB_I8x8, MB_I16x16, MB_IPCM, MB_P16x16, MB_P16x8, MB_P8x16, MB_P8x8, MB_PSKIP, MB_B, MB_BDIRECT, MB_BSKIP = range(13)  # H264MI_MB_*: values of the "type" plane
STREAM_DERIVED = 0x40000000                           # H264MI_STREAM_DERIVED: the pseudo-stream of the derived (deinterlaced) frames
_DEINT_NAMES = {"field": DEINT_FIELD, "blend": DEINT_BLEND, "edge": DEINT_EDGE}
_DEINT_MOTION_NAMES = {"motion": DEINT_FIELD, "motion_edge": DEINT_EDGE}  # the motion-adaptive modes of Decoder.deinterlace, by the spatial mode they pull from
DEINT_PREV_NONE, DEINT_PREV_HISTORY = -1, -2          # H264MI_DEINT_PREV_*: prev_frame of a motion-adaptive item / Decoder.derived_prev
DEINT_HISTORY = 1                                     # H264MI_DEINT_HISTORY: flag of h264mi_batch_deinterlace_motion (Decoder.deinterlace(history=True))
STATS_CELL_SUM, STATS_CELL_SAD = 1, 2                 # H264MI_STATS_CELL_*: planes of Decoder.stats_batch / stats_items / frame_stats
STATS_PLANE_NAMES = ("cell_sum", "cell_sad")          # ... by name, in the order they are written; STATS_PLANE_NAMES[i] is bit 1 << i
STATS_PREV_NONE, STATS_PREV_HISTORY = -1, -2          # H264MI_STATS_PREV_*: prev_frame of a statistics item
STATS_HISTORY = 1                                     # H264MI_STATS_HISTORY: flag of h264mi_batch_stats_plan / _device (history=True)
# the scalar fields of h264mi_frame_stats in record order: 8 x uint64 at byte 0, 8 x uint32 at byte 64; hist_y[256] follows at byte 96
STATS_U64 = ("sum_y", "sum_y2", "sum_cb", "sum_cr", "sad_y", "sse_y", "sad_cb", "sad_cr")
STATS_U32 = ("min_y", "max_y", "changed_y", "has_prev", "w", "h", "gw", "gh")
JPEG_RANGE_AUTO, JPEG_RANGE_KEEP, JPEG_RANGE_FULL = 0, 1, 2  # H264MI_JPEG_RANGE_*: `range` of Decoder.frames_jpeg / i420_jpeg ("auto", "keep", "full")
JPEG_TRUNCATED = 1                                    # H264MI_JPEG_TRUNCATED: status of an item that did not fit its slot
_JPEG_RANGE_NAMES = {"auto": JPEG_RANGE_AUTO, "keep": JPEG_RANGE_KEEP, "full": JPEG_RANGE_FULL}
_ECAPACITY = -7                                       # H264MI_ECAPACITY
_DT_NAMES = {"u8": DT_U8, "uint8": DT_U8, "f16": DT_F16, "float16": DT_F16, "bf16": DT_BF16, "bfloat16": DT_BF16, "f32": DT_F32, "float32": DT_F32}


def _fmt(fmt):
    if isinstance(fmt, str):
        if fmt.lower() not in _FMT_NAMES:
            raise H264MIError(-1, "unknown output format %r (i420, nv12, rgb24, rgbp)" % (fmt,))
        return _FMT_NAMES[fmt.lower()]
    return int(fmt)


def _filter(filter):
    if isinstance(filter, str):
        if filter.lower() not in _FILTER_NAMES:
            raise H264MIError(-1, "unknown scale filter %r (bilinear, area)" % (filter,))
        return _FILTER_NAMES[filter.lower()]
    return int(filter)


def side_planes(planes):
    """A set of H264MI_SIDE_* bits from an int or from plane names ("mvx0", "dpoc1", ...; SIDE_NAMES)."""
    if isinstance(planes, int):
        return planes
    bits = 0
    for name in ([planes] if isinstance(planes, str) else planes):
        if name not in SIDE_NAMES:
            raise H264MIError(-1, "unknown side-information plane %r (one of %s)" % (name, ", ".join(SIDE_NAMES)))
        bits |= 1 << SIDE_NAMES.index(name)
    return bits


def stats_planes(planes):
    """A set of H264MI_STATS_CELL_* bits from an int or from plane names ("cell_sum", "cell_sad"; STATS_PLANE_NAMES)."""
    if isinstance(planes, int):
        return planes
    bits = 0
    for name in planes:
        if name not in STATS_PLANE_NAMES:
            raise H264MIError(-1, "unknown statistics plane %r (one of %s)" % (name, ", ".join(STATS_PLANE_NAMES)))
        bits |= 1 << STATS_PLANE_NAMES.index(name)
    return bits


def stats_spec(cell=0, planes=0, thresh=0):
    """An h264mi_stats_spec: the cell size of the grid (0: none; 8, 16, 32, 64), its planes, and the threshold of changed_y."""
    return _lib.StatsSpec(int(cell), stats_planes(planes), int(thresh), 0)


def jpeg_spec(quality=90, range="auto", restart_mcus=0):
    """An h264mi_jpeg_spec: quality 1 .. 100, range "auto" / "keep" / "full" (or a JPEG_RANGE_* value), MCUs per restart interval (0: an MCU row)."""
    if isinstance(range, str):
        if range.lower() not in _JPEG_RANGE_NAMES:
            raise H264MIError(-1, "unknown JPEG range %r (one of %s)" % (range, ", ".join(_JPEG_RANGE_NAMES)))
        range = _JPEG_RANGE_NAMES[range.lower()]
    return _lib.JpegSpec(int(quality), int(range), int(restart_mcus), 0)


def jpeg_size(w, h, mono=False, quality=90, range="keep", restart_mcus=0):
    """(header_bytes, bound_bytes) of the JPEG file of a w x h frame (h264mi_jpeg_size): the length of SOI .. SOS, and an upper bound of any file of
    that shape -- a slot of bound_bytes never truncates."""
    hb, bb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    check(_lib.load().h264mi_jpeg_size(ctypes.byref(jpeg_spec(quality, range, restart_mcus)), int(w), int(h), int(bool(mono)), ctypes.byref(hb), ctypes.byref(bb)))
    return hb.value, bb.value


def jpeg_quant_table(quality, chroma=False):
    """The quantisation table of `quality` for luma or chroma, 64 values in natural order (h264mi_jpeg_quant_table)."""
    q = (ctypes.c_uint16 * 64)()
    check(_lib.load().h264mi_jpeg_quant_table(int(quality), int(bool(chroma)), q))
    return list(q)


def jpeg_block(samples, q):
    """The block rule (h264mi_jpeg_block): 64 samples and a table, natural order -> 64 levels."""
    s, t, lv = (ctypes.c_uint8 * 64)(*[int(v) for v in samples]), (ctypes.c_uint16 * 64)(*[int(v) for v in q]), (ctypes.c_int16 * 64)()
    check(_lib.load().h264mi_jpeg_block(s, t, lv))
    return list(lv)


def _deint(mode):
    if isinstance(mode, str):
        if mode.lower() not in _DEINT_NAMES:
            raise H264MIError(-1, "unknown deinterlace mode %r (field, blend, edge)" % (mode,))
        return _DEINT_NAMES[mode.lower()]
    return int(mode)


def deint_rows(mode, parity, n_rows, y):
    """The deinterlacing rule of include/h264mi.h for row y of a plane of n_rows rows, from the library (h264mi_deint_rows; no GPU): (kept, up, dn)."""
    v = [ctypes.c_int32(0) for _ in range(3)]
    check(_lib.load().h264mi_deint_rows(_deint(mode), int(parity), n_rows, y, *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def deint_motion_pixel(s, p, sp):
    """The motion-adaptive rule of include/h264mi.h for one sample, from the library (h264mi_deint_motion_pixel; no GPU): s and p are the samples of the
    source and of the predecessor at rows (up, y, dn), p = None: no predecessor; sp is the spatial value."""
    out = ctypes.c_int32(0)
    a3 = ctypes.c_uint8 * 3
    check(_lib.load().h264mi_deint_motion_pixel(a3(*s), None if p is None else a3(*p), int(sp), ctypes.byref(out)))
    return out.value


def _dtype(dtype):
    """An H264MI_DT_* value from a name ("u8", "f16", "bf16", "f32", "float16", ...), a torch or numpy dtype, or the value itself."""
    if isinstance(dtype, int):
        return dtype
    name = str(dtype).lower().replace("torch.", "").replace("<class 'numpy.", "").replace("'>", "")
    if name not in _DT_NAMES:
        raise H264MIError(-1, "unknown tensor dtype %r (u8, f16, bf16, f32)" % (dtype,))
    return _DT_NAMES[name]


def fit_rect(fit, w, h, out_w, out_h):
    """Where a w x h source goes in an out_w x out_h canvas, from the library (h264mi_fit_rect; no GPU): (px, py, sw, sh).  fit: FIT_STRETCH or
    FIT_LETTERBOX (the aspect ratio kept to the nearest pixel, centred)."""
    v = [ctypes.c_int32(0) for _ in range(4)]
    check(_lib.load().h264mi_fit_rect(int(fit), w, h, out_w, out_h, *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def tensor_spec(size, fmt="rgbp", dtype="f32", csc=0, filter="bilinear", letterbox=False, bgr=False, pad=(114, 114, 114), scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
    """An h264mi_tensor_spec: canvas size = (out_w, out_h), layout "rgbp" (CHW) or "rgb24" (HWC), element type, csc and filter as for scale_batch,
    stretch or letterbox, RGB or BGR channel order, the padding colour (R, G, B bytes), and scale / bias per colour (R, G, B): an 8-bit value v
    becomes float32(float32(v * scale) + bias), then the element type."""
    sp = _lib.TensorSpec()
    sp.format, sp.dtype, sp.csc, sp.filter = _fmt(fmt), _dtype(dtype), int(csc), _filter(filter)
    sp.out_w, sp.out_h = int(size[0]), int(size[1])
    sp.fit, sp.flags = (FIT_LETTERBOX if letterbox else FIT_STRETCH), (TENSOR_BGR if bgr else 0)
    for c in range(3):
        sp.pad[c], sp.scale[c], sp.bias[c] = int(pad[c]), float(scale[c]), float(bias[c])
    return sp


def scale_taps(filter, n_in, n_out, i):
    """The scaling rule of include/h264mi.h for output index i of an axis of n_in samples scaled to n_out, from the library (h264mi_scale_taps; no
    GPU): ([source indices], [weights]).  Bilinear: two taps with weights (256 - f, f); area: the overlapping source samples and their overlaps."""
    L = _lib.load()
    first, count = ctypes.c_int32(0), ctypes.c_int32(0)
    one = (ctypes.c_int32 * 2)()
    code = L.h264mi_scale_taps(_filter(filter), n_in, n_out, i, ctypes.byref(first), ctypes.byref(count), one, 2)
    w = one
    if code == -7:  # H264MI_ECAPACITY: *count says how many there are
        w = (ctypes.c_int32 * count.value)()
        code = L.h264mi_scale_taps(_filter(filter), n_in, n_out, i, ctypes.byref(first), ctypes.byref(count), w, count.value)
    check(code)
    return [min(first.value + t, n_in - 1) for t in range(count.value)], [w[t] for t in range(count.value)]


def _frames_with_headroom(frames_per_batch, conceal_errors):
    """max_frames_per_batch of a decoder fed chunks of `frames_per_batch` pictures: frames inserted for lost pictures need room in a full chunk too."""
    return frames_per_batch + (CONCEAL_MAX_GAP if int(conceal_errors) & CONCEAL_PICTURES else 0)


class Decoder:
    """Batched GPU decoder: N independent Annex-B streams side by side on one MI355X."""

    def __init__(self, max_streams=1, max_width=1920, max_height=1088, max_frames_per_batch=32, max_slices_per_frame=8, device=0,
                 max_bitstream_bytes=0, hip_stream=None, max_ref_frames=0, coef_blocks_per_mb=0, b_pictures=0, allow_unpinned_field_cabac=0,
                 conceal_errors=False):
        L = _lib.load()
        cfg = _lib.Config()
        cfg.struct_size = ctypes.sizeof(cfg)
        cfg.b_pictures = b_pictures  # 1: the B-only buffers exist from the start (default: from the first B slice on)
        cfg.allow_unpinned_field_cabac = allow_unpinned_field_cabac  # 1: CABAC field pictures are decoded with the unpinned context tables of field-coded blocks (default: refused)
        # True / CONCEAL_SLICES: lost macroblocks of non-IDR frame pictures are copied from a reference picture and the stream goes on (default: the
        # stream waits for an IDR picture); | CONCEAL_PICTURES: wholly lost reference frames are inserted as copies too; | CONCEAL_FIELDS: field pictures too;
        # | CONCEAL_IDR: IDR frame pictures that still have a reference frame too (they are then reconstructed behind that frame when one batch holds both);
        # | CONCEAL_LONE_FIELDS (with CONCEAL_FIELDS): the wholly lost field of a frame coded as two field pictures is inserted as a copy too
        cfg.conceal_errors = int(conceal_errors)
        cfg.device, cfg.max_streams, cfg.max_width, cfg.max_height = device, max_streams, max_width, max_height
        cfg.max_frames_per_batch, cfg.max_slices_per_frame, cfg.max_bitstream_bytes = max_frames_per_batch, max_slices_per_frame, max_bitstream_bytes
        cfg.hip_stream = hip_stream
        cfg.max_ref_frames, cfg.coef_blocks_per_mb = max_ref_frames, coef_blocks_per_mb  # 0: defaults (16 reference slots, 8 blocks per macroblock)
        self._h = ctypes.c_void_p()
        check(L.h264mi_decoder_create(ctypes.byref(cfg), ctypes.byref(self._h)))
        self._L = L
        self.max_streams = max_streams
        self.device = device
        self._keep = None

    def close(self):
        if self._h:
            self._L.h264mi_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream):
        check(self._L.h264mi_decoder_set_stream(self._h, hip_stream))

    def reset(self):
        check(self._L.h264mi_decoder_reset(self._h))

    def reset_stream(self, stream):
        """Forget parameter sets, reference pictures and POC history of one stream slot (a new connection takes it over)."""
        check(self._L.h264mi_stream_reset(self._h, stream))

    def set_isolation(self, on=True):
        """With isolation a broken stream is dropped from the batch and marked instead of failing prepare() / sync()."""
        check(self._L.h264mi_decoder_set_isolation(self._h, int(on)))

    def set_random_access(self, mode=True):
        """True / RA_RECOVERY_POINT: a stream that has decoded nothing yet, or that an error took out, starts at its next IDR picture OR at its next
        non-IDR picture with a recovery point SEI message of recovery_frame_cnt 0; the slices in front of it are skipped without an error, the
        pictures that precede the entry picture in output order (leading pictures) are dropped.  False (default): IDR pictures only.  From the
        next prepare() on."""
        check(self._L.h264mi_decoder_set_random_access(self._h, int(mode)))

    def frame_entry(self, stream, frame):
        """h264mi_frame_entry_info of a decoded frame: the recovery point SEI message of its access unit (recovery_point, recovery_frame_cnt,
        exact_match_flag, broken_link_flag, changing_slice_group_idc; either mode) and `entry`: the stream entered here after waiting."""
        fe = _lib.FrameEntryInfo()
        check(self._L.h264mi_frame_entry(self._h, stream, frame, ctypes.byref(fe)))
        return fe

    def random_access_stats(self, stream=0):
        """(entries, skipped_waiting_nals, skipped_leading_pictures) of a stream since it was created / reset_stream(): non-IDR entry points taken,
        slice NAL units skipped while it waited for one, leading pictures dropped."""
        s = _lib.RandomAccessStats()
        check(self._L.h264mi_stream_random_access_stats(self._h, stream, ctypes.byref(s)))
        return s.entries, s.skipped_waiting_nals, s.skipped_leading_pictures

    def stream_status(self, stream):
        st = ctypes.c_int32(0)
        check(self._L.h264mi_stream_status(self._h, stream, ctypes.byref(st)))
        return st.value

    def frame_info(self, stream, frame):
        """h264mi_frame_info of a decoded frame: display / coded size, crop origin, PicOrderCnt, frame_num, nal_ref_idc, idr."""
        fi = _lib.FrameInfo()
        check(self._L.h264mi_frame_get_info(self._h, stream, frame, ctypes.byref(fi)))
        return fi

    def device_bytes(self):
        """Device memory the decoder holds right now (h264mi_decoder_memory)."""
        n = ctypes.c_int64()
        check(self._L.h264mi_decoder_memory(self._h, ctypes.byref(n)))
        return int(n.value)

    def unpinned_failures(self):
        """Slices of CABAC field pictures that failed in the entropy kernels so far (h264mi_decoder_unpinned_failures)."""
        n = ctypes.c_int64()
        check(self._L.h264mi_decoder_unpinned_failures(self._h, ctypes.byref(n)))
        return n.value

    def frame_concealed(self, stream, frame):
        """Concealed macroblocks of a frame of the last batch (h264mi_frame_concealed); call after sync()."""
        n = ctypes.c_int32()
        check(self._L.h264mi_frame_concealed(self._h, stream, frame, ctypes.byref(n)))
        return int(n.value)

    def concealed(self):
        """(slices, macroblocks) concealed since the decoder was created (h264mi_decoder_concealed)."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        check(self._L.h264mi_decoder_concealed(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def concealed_pictures(self):
        """Frames inserted for wholly lost pictures since the decoder was created (h264mi_decoder_concealed_pictures)."""
        n = ctypes.c_int64()
        check(self._L.h264mi_decoder_concealed_pictures(self._h, ctypes.byref(n)))
        return int(n.value)

    def concealed_fields(self):
        """Fields inserted for wholly lost fields since the decoder was created (h264mi_decoder_concealed_fields)."""
        n = ctypes.c_int64()
        check(self._L.h264mi_decoder_concealed_fields(self._h, ctypes.byref(n)))
        return int(n.value)

    def coef_pool(self):
        """(used, capacity) of the residual-coefficient pool in 32-byte blocks (h264mi_decoder_coef_pool); call after sync()."""
        u, c = ctypes.c_int64(), ctypes.c_int64()
        check(self._L.h264mi_decoder_coef_pool(self._h, ctypes.byref(u), ctypes.byref(c)))
        return int(u.value), int(c.value)

    def set_profiling(self, on=True):
        check(self._L.h264mi_decoder_set_profiling(self._h, int(on)))

    def kernel_times_ms(self):
        a = (ctypes.c_double * 5)()
        check(self._L.h264mi_last_kernel_times(self._h, a))
        return dict(zip(("entropy", "inter", "intra", "deblock", "total"), list(a)))

    def launch_times_ms(self, kernel):
        """Duration of every launch of `kernel` ("entropy", "inter", "intra", "deblock") in the last profiled pass."""
        k = ("entropy", "inter", "intra", "deblock").index(kernel)
        n = ctypes.c_int32(0)
        check(self._L.h264mi_last_launch_times(self._h, k, None, 0, ctypes.byref(n)))
        a = (ctypes.c_float * max(n.value, 1))()
        check(self._L.h264mi_last_launch_times(self._h, k, a, n.value, ctypes.byref(n)))
        return list(a)[:n.value]

    def _args(self, streams):
        n = len(streams)
        bufs = (ctypes.c_void_p * n)()
        lens = (ctypes.c_size_t * n)()
        keep = []
        for i, s in enumerate(streams):
            if s:
                b = ctypes.create_string_buffer(bytes(s), len(s))
                keep.append(b)
                bufs[i] = ctypes.cast(b, ctypes.c_void_p)
                lens[i] = len(s)
        self._keep = keep
        return n, bufs, lens

    def prepare(self, streams):
        n, bufs, lens = self._args(streams)
        info = _lib.BatchInfo()
        check(self._L.h264mi_batch_prepare(self._h, n, bufs, lens, ctypes.byref(info)))
        self.info = info
        return info

    def execute(self):
        check(self._L.h264mi_batch_execute(self._h))

    def sync(self):
        check(self._L.h264mi_batch_sync(self._h))

    def decode(self, streams):
        """prepare + execute + sync; returns the batch info."""
        info = self.prepare(streams)
        self.execute()
        self.sync()
        return info

    def frame_count(self, stream=0):
        n = ctypes.c_int32(0)
        check(self._L.h264mi_stream_frame_count(self._h, stream, ctypes.byref(n)))
        return n.value

    def frame_planes(self, stream, frame):
        y, cb, cr = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        py, pc, w, h = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        check(self._L.h264mi_frame_device_planes(self._h, stream, frame, ctypes.byref(y), ctypes.byref(cb), ctypes.byref(cr), ctypes.byref(py),
                                                 ctypes.byref(pc), ctypes.byref(w), ctypes.byref(h)))
        return dict(y=y.value, cb=cb.value, cr=cr.value, pitch_y=py.value, pitch_c=pc.value, coded_width=w.value, coded_height=h.value)

    @staticmethod
    def i420_size(w, h):
        """H264MI_I420_SIZE of include/h264mi.h: w*h luma bytes, then two chroma planes of ceil(w/2) x ceil(h/2) (w*h*3/2 for even sizes;
        the display size of a monochrome stream may be odd)."""
        return w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)

    def read_frame(self, stream, frame, crop=True):
        fi = self.frame_info(stream, frame)
        buf = np.zeros(fi.coded_width * fi.coded_height * 3 // 2, dtype=np.uint8)
        check(self._L.h264mi_frame_read(self._h, stream, frame, int(crop), buf.ctypes.data, buf.nbytes))
        return buf

    def read_frame_tight(self, stream, frame, crop=True):
        """The frame as exactly i420_size(w, h) bytes of its own geometry (display size when cropped)."""
        fi = self.frame_info(stream, frame)
        w, h = (fi.width, fi.height) if crop else (fi.coded_width, fi.coded_height)
        return self.read_frame(stream, frame, crop)[:self.i420_size(w, h)]

    def read_frames(self, stream=0, crop=False, size=None):
        """All frames of `stream` from the last batch as uint8[n, w*h*3/2] (tight I420)."""
        n = self.frame_count(stream)
        out = []
        for f in range(n):
            b = self.read_frame(stream, f, crop)
            out.append(b if size is None else b[:size])
        return np.stack(out) if out else np.zeros((0, 0), np.uint8)

    def pack_batch(self, dst_ptr, cap, stream=-1):
        """K6 in one launch: every frame of the last executed batch (of one stream, or of all streams) cropped and packed
        back to back as tight I420 into the DEVICE buffer at dst_ptr.  Returns the number of bytes."""
        n = ctypes.c_size_t(0)
        check(self._L.h264mi_batch_pack_device(self._h, stream, dst_ptr, cap, ctypes.byref(n)))
        return n.value

    @staticmethod
    def output_size(fmt, w, h):
        """Bytes of a w x h frame in `fmt` ("i420", "nv12", "rgb24", "rgbp" or an H264MI_FMT_* value): h264mi_output_size."""
        n = ctypes.c_size_t(0)
        check(_lib.load().h264mi_output_size(_fmt(fmt), w, h, ctypes.byref(n)))
        return n.value

    def frame_colour(self, stream, frame):
        """(matrix_coefficients, video_full_range) of the SPS the frame was decoded under -- (2, 0) where it carries none: what CSC_AUTO resolves from."""
        m, f = ctypes.c_int32(0), ctypes.c_int32(0)
        check(self._L.h264mi_frame_colour(self._h, stream, frame, ctypes.byref(m), ctypes.byref(f)))
        return m.value, f.value

    def frame_fields(self, stream, frame):
        """What the frame's fields are (h264mi_frame_fields): field_coded (coded as two field pictures), top_field_order_cnt, bottom_field_order_cnt,
        first_parity (1: the bottom field comes first)."""
        ff = _lib.FieldInfo()
        check(self._L.h264mi_frame_fields(self._h, stream, frame, ctypes.byref(ff)))
        return ff

    def deinterlace(self, stream=-1, mode="field", rate=1, items=None, history=False):
        """K10 in one launch: derived (deinterlaced) frames of the last executed batch, which REPLACE the decoder's list of derived frames and are then
        frames 0 .. n - 1 of the pseudo-stream STREAM_DERIVED for frame_count, frame_info, frame_colour, frame_fields, read_frame(crop=True) and every
        pack / convert / scale / tensor call.  mode: "field", "blend" or "edge".  Without `items`: every frame of `stream` (-1: of all streams,
        stream-major); rate 1: one derived frame per frame, of its first parity; rate 2: two, the first parity then the other ("bob"; not for "blend").
        items: a list of (stream, frame, parity) with parity 0 (top), 1 (bottom) or DEINT_PARITY_FIRST; an empty list empties the list of derived
        frames.  execute(), reset() and reset_stream() empty it too.  Returns the number of derived frames.
        mode "motion" or "motion_edge": motion-adaptive ("Motion-adaptive deinterlacing" of include/h264mi.h), pulling from "field" or "edge".  Without
        `items` a frame's predecessor is the frame before it in output order; history=True gives the first one the stream's history, if the batch
        before left a valid one, and takes this batch's.  items are then (stream, frame, parity, prev_frame), prev_frame a frame of the same stream,
        DEINT_PREV_NONE or DEINT_PREV_HISTORY."""
        n = ctypes.c_int32(0)
        if isinstance(mode, str) and mode.lower() in _DEINT_MOTION_NAMES:
            m = _DEINT_MOTION_NAMES[mode.lower()]
            if items is None:
                check(self._L.h264mi_batch_deinterlace_motion(self._h, stream, m, int(rate), DEINT_HISTORY if history else 0, ctypes.byref(n)))
                return n.value
            if history:
                raise ValueError("deinterlace: history goes with the batch form; an item names DEINT_PREV_HISTORY itself")
            arr = (_lib.DeintMotionItem * max(len(items), 1))()
            for a, it in zip(arr, items):
                a.stream, a.frame, a.parity, a.prev_frame = (int(v) for v in it)
            check(self._L.h264mi_items_deinterlace_motion(self._h, m, arr, len(items), ctypes.byref(n)))
            return n.value
        if history:
            raise ValueError("deinterlace: history needs mode \"motion\" or \"motion_edge\"")
        if items is None:
            check(self._L.h264mi_batch_deinterlace(self._h, stream, _deint(mode), int(rate), ctypes.byref(n)))
            return n.value
        arr = (_lib.DeintItem * max(len(items), 1))()
        for a, it in zip(arr, items):
            a.stream, a.frame, a.parity = (int(v) for v in it)
        check(self._L.h264mi_items_deinterlace(self._h, _deint(mode), arr, len(items), ctypes.byref(n)))
        return n.value

    def derived_prev(self, k):
        """What derived frame k was made from besides its source (h264mi_derived_prev): a frame index of the source's stream, DEINT_PREV_NONE (also for
        every frame of "field", "blend" and "edge") or DEINT_PREV_HISTORY."""
        v = ctypes.c_int32(0)
        check(self._L.h264mi_derived_prev(self._h, int(k), ctypes.byref(v)))
        return v.value

    def convert_frame(self, stream, frame, dst_ptr, cap, fmt, csc=0):
        """K7 for one frame of the last executed batch: cropped and converted to `fmt` into the DEVICE buffer at dst_ptr (asynchronous on the
        decoder's stream).  csc: CSC_AUTO / CSC_BT601 / CSC_BT709, | CSC_FULL_RANGE (explicit matrix only), | CSC_CHROMA_BILINEAR; 0 for "nv12"."""
        check(self._L.h264mi_frame_convert_device(self._h, stream, frame, _fmt(fmt), csc, dst_ptr, cap))

    def convert_batch(self, dst_ptr, cap, fmt, csc=0, stream=-1):
        """K7 in one launch: every frame of the last executed batch (of one stream, or of all streams, stream-major) cropped and converted to
        `fmt`, back to back in the DEVICE buffer at dst_ptr -- pack_batch's contract.  Returns the number of bytes."""
        n = ctypes.c_size_t(0)
        check(self._L.h264mi_batch_convert_device(self._h, stream, _fmt(fmt), csc, dst_ptr, cap, ctypes.byref(n)))
        return n.value

    def scale_frame(self, stream, frame, dst_ptr, cap, fmt, size, csc=0, filter="bilinear"):
        """K8 for one frame of the last executed batch: cropped, scaled to size = (ow, oh) and converted to `fmt` ("i420" too) into the DEVICE buffer
        at dst_ptr (asynchronous on the decoder's stream).  filter: "bilinear" or "area" (downscaling only); csc as for convert_frame."""
        check(self._L.h264mi_frame_scale_device(self._h, stream, frame, _fmt(fmt), csc, int(size[0]), int(size[1]), _filter(filter), dst_ptr, cap))

    def scale_batch(self, dst_ptr, cap, fmt, size, csc=0, filter="bilinear", stream=-1):
        """K8 in one launch: every frame of the last executed batch (of one stream, or of all streams, stream-major) cropped, scaled to
        size = (ow, oh) whatever its display size, and converted to `fmt`, back to back in the DEVICE buffer at dst_ptr -- convert_batch's contract.
        Returns the number of bytes: frames x output_size(fmt, ow, oh)."""
        n = ctypes.c_size_t(0)
        check(self._L.h264mi_batch_scale_device(self._h, stream, _fmt(fmt), csc, int(size[0]), int(size[1]), _filter(filter), dst_ptr, cap, ctypes.byref(n)))
        return n.value

    @staticmethod
    def tensor_size(spec):
        """Bytes of one tensor item of `spec` (tensor_spec(...)): h264mi_tensor_size, which validates the spec."""
        n = ctypes.c_size_t(0)
        check(_lib.load().h264mi_tensor_size(ctypes.byref(spec), ctypes.byref(n)))
        return n.value

    def tensor_batch(self, dst_ptr, cap, spec, stream=-1):
        """K9 in one launch: the whole of every frame of the last executed batch (of one stream, or of all streams, stream-major) as a tensor item of
        `spec`, back to back in the DEVICE buffer at dst_ptr -- scale_batch's contract.  Returns the number of bytes: frames x tensor_size(spec)."""
        n = ctypes.c_size_t(0)
        check(self._L.h264mi_batch_tensor_device(self._h, stream, ctypes.byref(spec), dst_ptr, cap, ctypes.byref(n)))
        return n.value

    def tensor_items(self, dst_ptr, cap, spec, items):
        """K9 in one launch over a list of items (stream, frame, x, y, w, h): the region (x, y, w, h) of that frame of the last executed batch, in
        display coordinates with an even origin (w = h = 0: the whole frame), as a tensor item of `spec`; item order, back to back.  The same frame may
        appear in many items.  Returns the number of bytes."""
        arr = (_lib.TensorItem * max(len(items), 1))()
        for a, it in zip(arr, items):
            a.stream, a.frame, a.x, a.y, a.w, a.h = (int(v) for v in it)
        n = ctypes.c_size_t(0)
        check(self._L.h264mi_items_tensor_device(self._h, ctypes.byref(spec), arr, len(items), dst_ptr, cap, ctypes.byref(n)))
        return n.value

    def _model_tensor(self, stream, fmt, csc, size, filter, dtype, scale, bias, mean, std, letterbox, pad, rois, bgr):
        """frames_tensor with one of the model-input keywords: one K9 launch."""
        import torch
        if size is None:
            raise ValueError("frames_tensor: dtype, scale, bias, mean, std, letterbox, rois and bgr need a size")
        dt = _dtype("u8" if dtype is None else dtype)
        if (mean is not None or std is not None) and (scale is not None or bias is not None):
            raise ValueError("frames_tensor: give mean / std or scale / bias, not both")
        if mean is not None or std is not None:
            if dt == DT_U8:
                raise ValueError("frames_tensor: mean / std need a float dtype")
            mean, std = (0.0, 0.0, 0.0) if mean is None else mean, (1.0, 1.0, 1.0) if std is None else std
            scale = [1.0 / (255.0 * float(std[c])) for c in range(3)]   # Python doubles, rounded to float32 once (by the ctypes field)
            bias = [-float(mean[c]) / float(std[c]) for c in range(3)]
        spec = tensor_spec(size, fmt, dt, csc, filter, letterbox, bgr, pad, (1.0, 1.0, 1.0) if scale is None else scale, (0.0, 0.0, 0.0) if bias is None else bias)
        one = self.tensor_size(spec)
        if rois is not None:
            n = len(rois)
        else:
            n = sum(self.frame_count(s) for s in (range(self.max_streams) if stream < 0 else (stream,)))
        ow, oh = spec.out_w, spec.out_h
        tdt = {DT_U8: torch.uint8, DT_F16: torch.float16, DT_BF16: torch.bfloat16, DT_F32: torch.float32}[dt]
        out = torch.empty((n, oh, ow, 3) if spec.format == FMT_RGB24 else (n, 3, oh, ow), dtype=tdt, device="cuda:%d" % self.device)
        if n:
            torch.cuda.current_stream(out.device).synchronize()  # whatever still uses a recycled block has finished before K9 writes it
            cap = out.numel() * out.element_size()
            got = self.tensor_items(out.data_ptr(), cap, spec, rois) if rois is not None else self.tensor_batch(out.data_ptr(), cap, spec, stream)
            assert got == cap == n * one
            self.sync()
        return out

    def frames_tensor(self, stream, fmt="rgbp", csc=0, size=None, filter="bilinear", *, dtype=None, scale=None, bias=None, mean=None, std=None,
                      letterbox=False, pad=(114, 114, 114), rois=None, bgr=False, deinterlace=None, field_rate=False, deinterlace_history=False):
        """The frames of `stream` of the last executed batch as one torch uint8 tensor on the decoder's device: [n, 3, h, w] ("rgbp"), [n, h, w, 3]
        ("rgb24") or [n, H264MI_I420_SIZE(w, h)] ("nv12"), converted by one K7 launch.  Raises ValueError if the stream's frames differ in display size.
        With size = (ow, oh) the frames are scaled to that size by one K8 launch (`filter`: "bilinear" or "area"): the shapes are those with (ow, oh) for
        (w, h), "i420" is a format too ([n, H264MI_I420_SIZE(ow, oh)]), frames of unlike display size are fine, and stream = -1 takes the frames of all
        streams, stream-major.
        Ordering, both ways, by synchronising (no event is involved): the tensor comes from torch's caching allocator on torch's current stream, which may
        hand back a block that work still queued on that stream reads, and the conversion writes it on the decoder's stream -- so torch's current
        stream is SYNCHRONISED after the allocation and before the launch; and the decoder's stream is SYNCHRONISED (sync()) before the method returns,
        so the tensor is complete for any torch stream.  A caller who cannot afford the two waits allocates for themselves and calls convert_batch
        or scale_batch.
        Model input (one K9 launch instead; `size` is required; the same two synchronisations): with any of the keyword-only arguments set the result
        is [n, 3, oh, ow] ("rgbp") or [n, oh, ow, 3] ("rgb24") of torch dtype `dtype` (torch.uint8 / float16 / bfloat16 / float32 or "u8", "f16", "bf16",
        "f32"; default uint8).  An 8-bit value v of colour c becomes float32(float32(v * scale[c]) + bias[c]) rounded to `dtype`; mean / std (per colour,
        in 0 .. 1) stand for scale[c] = float32(1.0 / (255.0 * std[c])) and bias[c] = float32(-mean[c] / std[c]), evaluated in Python doubles and
        rounded once -- giving both forms, or mean / std with uint8, is a ValueError.  letterbox keeps the aspect ratio and fills the rest of the canvas
        with pad = (R, G, B); bgr writes the channels in the order B, G, R (scale, bias, mean, std and pad stay per colour R, G, B).  rois, a list of
        (stream, frame, x, y, w, h) regions in display coordinates with even origins (w = h = 0: the whole frame), replaces "all frames of `stream`":
        n = len(rois), in list order.
        deinterlace = "field", "blend" or "edge" (keyword-only): the frames of `stream` are deinterlaced first (one K10 launch: self.deinterlace(stream,
        mode, rate), which replaces the decoder's derived frames) and everything above is then done for the pseudo-stream STREAM_DERIVED; field_rate
        makes that two frames per frame, the first field's then the second's.  rois then name frames of STREAM_DERIVED.  deinterlace = "motion" or
        "motion_edge" is the motion-adaptive route of self.deinterlace, and deinterlace_history its history=True: the first frame in output order is
        pulled from the last frame of the batch before."""
        import torch
        f = _fmt(fmt)
        if deinterlace is not None:
            self.deinterlace(stream, deinterlace, 2 if field_rate else 1, history=deinterlace_history)
            stream = STREAM_DERIVED
        elif field_rate or deinterlace_history:
            raise ValueError("frames_tensor: field_rate and deinterlace_history need deinterlace")
        if dtype is not None or scale is not None or bias is not None or mean is not None or std is not None or letterbox or rois is not None or bgr:
            return self._model_tensor(stream, f, csc, size, filter, dtype, scale, bias, mean, std, letterbox, pad, rois, bgr)
        if size is not None:
            ow, oh = int(size[0]), int(size[1])
            n = sum(self.frame_count(s) for s in (range(self.max_streams) if stream < 0 else (stream,)))
            shape = {FMT_I420: (n, self.i420_size(ow, oh)), FMT_NV12: (n, self.i420_size(ow, oh)), FMT_RGB24: (n, oh, ow, 3), FMT_RGBP: (n, 3, oh, ow)}.get(f)
            if shape is None:
                raise H264MIError(-1, "frames_tensor: format %r is not i420, nv12, rgb24 or rgbp" % (fmt,))
            out = torch.empty(shape, dtype=torch.uint8, device="cuda:%d" % self.device)
            if n:
                torch.cuda.current_stream(out.device).synchronize()  # whatever still uses a recycled block has finished before K8 writes it
                got = self.scale_batch(out.data_ptr(), out.numel(), f, (ow, oh), csc, filter, stream)
                assert got == out.numel()
                self.sync()
            return out
        n = self.frame_count(stream)
        infos = [self.frame_info(stream, i) for i in range(n)]
        sizes = {(fi.width, fi.height) for fi in infos}
        if len(sizes) > 1:
            raise ValueError("the frames of stream %d differ in display size (%s): convert them with convert_frame / convert_batch" % (stream, sorted(sizes)))
        w, h = sizes.pop() if sizes else (0, 0)
        shape = {FMT_NV12: (n, self.i420_size(w, h)), FMT_RGB24: (n, h, w, 3), FMT_RGBP: (n, 3, h, w)}.get(f)
        if shape is None:
            raise H264MIError(-1, "frames_tensor: format %r is not nv12, rgb24 or rgbp" % (fmt,))
        out = torch.empty(shape, dtype=torch.uint8, device="cuda:%d" % self.device)
        if n:
            torch.cuda.current_stream(out.device).synchronize()  # whatever still uses a recycled block has finished before K7 writes it
            got = self.convert_batch(out.data_ptr(), out.numel(), f, csc, stream)
            assert got == out.numel()
            self.sync()
        return out

    @staticmethod
    def side_size(planes, w, h):
        """(gw, gh, bytes) of the side information of one w x h frame: a grid of ceil(w / 4) x ceil(h / 4) cells, one int16 plane per selected plane
        (h264mi_side_size)."""
        gw, gh, n = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_size_t(0)
        check(_lib.load().h264mi_side_size(side_planes(planes), w, h, ctypes.byref(gw), ctypes.byref(gh), ctypes.byref(n)))
        return gw.value, gh.value, n.value

    def ref_pocs(self, stream, frame, slice, list):
        """(cur_poc, [PicOrderCnt of every active entry of RefPicList`list`]) of slice `slice` (its ordinal in the picture: the "slice" plane; -1: the
        concealment pseudo-slice) of a frame of the last executed batch, as of list-building time (h264mi_frame_ref_pocs)."""
        cur, n = ctypes.c_int32(0), ctypes.c_int32(0)
        pocs = (ctypes.c_int32 * 32)()
        check(self._L.h264mi_frame_ref_pocs(self._h, stream, frame, slice, list, ctypes.byref(cur), pocs, 32, ctypes.byref(n)))
        return cur.value, [pocs[i] for i in range(n.value)]

    def side_batch(self, dst_ptr, cap, planes, stream=-1):
        """K11 in one launch: the macroblock side information (motion vectors, reference indices and picture order count distances, macroblock
        classes, QP, coded-block flags, slice ordinals; include/h264mi.h) of every frame of the last executed batch (of one stream, or of all streams,
        stream-major), per 4x4 luma block of the display rectangle, the selected planes in ascending bit order as tight int16 planes, frames back to
        back in the DEVICE buffer at dst_ptr.  Returns the number of bytes."""
        n = ctypes.c_size_t(0)
        check(self._L.h264mi_batch_side_device(self._h, stream, side_planes(planes), dst_ptr, cap, ctypes.byref(n)))
        return n.value

    def side_items(self, dst_ptr, cap, planes, items):
        """K11 in one launch over a list of (stream, frame) items of the last executed batch, in item order; the same frame may appear several times.
        Returns the number of bytes."""
        arr = (_lib.SideItem * max(len(items), 1))()
        for a, it in zip(arr, items):
            a.stream, a.frame = (int(v) for v in it)
        n = ctypes.c_size_t(0)
        check(self._L.h264mi_items_side_device(self._h, side_planes(planes), arr, len(items), dst_ptr, cap, ctypes.byref(n)))
        return n.value

    def side_info(self, stream=-1, planes=SIDE_NAMES, items=None):
        """The side information of the frames of `stream` (-1: of all streams, stream-major) of the last executed batch, or of the (stream, frame)
        `items`, as a list of torch int16 views [C, gh, gw] -- one per frame, C planes in ascending bit order (SIDE_NAMES) -- of ONE device tensor
        filled by one K11 launch.  Synchronises like frames_tensor: torch's current stream before the launch, the decoder's stream after it."""
        import torch
        bits = side_planes(planes)
        c = bin(bits).count("1")
        frames = list(items) if items is not None else [(s, f) for s in (range(self.max_streams) if stream < 0 else (stream,)) for f in range(self.frame_count(s))]
        shapes = []
        for s, f in frames:
            fi = self.frame_info(s, f)
            gw, gh, _ = self.side_size(bits, fi.width, fi.height)
            shapes.append((c, gh, gw))
        total = sum(a * b * w for a, b, w in shapes)
        out = torch.empty(total, dtype=torch.int16, device="cuda:%d" % self.device)
        if total:
            torch.cuda.current_stream(out.device).synchronize()  # whatever still uses a recycled block has finished before K11 writes it
            got = self.side_items(out.data_ptr(), 2 * total, bits, frames)
            assert got == 2 * total
            self.sync()
        views, at = [], 0
        for shp in shapes:
            n = shp[0] * shp[1] * shp[2]
            views.append(out[at:at + n].view(shp))
            at += n
        return views

    @staticmethod
    def stats_size(w, h, cell=0, planes=0, thresh=0):
        """(gw, gh, bytes) of the statistics item of one w x h frame: the 1120-byte record and, behind it, one uint32 plane of ceil(h / cell) x
        ceil(w / cell) cells per selected plane, rounded up to 16 bytes (h264mi_stats_size)."""
        gw, gh, n = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_size_t(0)
        check(_lib.load().h264mi_stats_size(ctypes.byref(stats_spec(cell, planes, thresh)), w, h, ctypes.byref(gw), ctypes.byref(gh), ctypes.byref(n)))
        return gw.value, gh.value, n.value

    def stats_plan(self, stream=-1, history=False):
        """The (stream, frame, prev_frame) items stats_batch would use (h264mi_batch_stats_plan; no device work): every frame of `stream` (-1: of all
        streams, stream-major) in decoding order against the frame before it in output order, STATS_PREV_NONE, or -- the first one, with history=True
        and a valid history -- STATS_PREV_HISTORY."""
        n = ctypes.c_int32(0)
        flags = STATS_HISTORY if history else 0
        code = self._L.h264mi_batch_stats_plan(self._h, stream, flags, None, 0, ctypes.byref(n))
        if code != _ECAPACITY:
            check(code)
        arr = (_lib.StatsItem * max(n.value, 1))()
        check(self._L.h264mi_batch_stats_plan(self._h, stream, flags, arr, n.value, ctypes.byref(n)))
        return [(a.stream, a.frame, a.prev_frame) for a in arr[:n.value]]

    def stats_batch(self, dst_ptr, cap, stream=-1, cell=0, planes=0, thresh=0, history=False):
        """K12 in one launch: the frame statistics ("Frame statistics" of include/h264mi.h) of every frame of the last executed batch (of one stream, or
        of all streams, stream-major) against the frame before it in output order, items back to back in the DEVICE buffer at dst_ptr (16-byte aligned).
        history=True gives each stream's first frame the stream's statistics history, if the batch before took one, and takes one.  Returns the number
        of bytes."""
        n = ctypes.c_size_t(0)
        check(self._L.h264mi_batch_stats_device(self._h, stream, ctypes.byref(stats_spec(cell, planes, thresh)), STATS_HISTORY if history else 0, dst_ptr, cap, ctypes.byref(n)))
        return n.value

    def stats_items(self, dst_ptr, cap, items, cell=0, planes=0, thresh=0):
        """K12 in one launch over a list of (stream, frame, prev_frame) items of the last executed batch, in item order; prev_frame is a frame of the same
        stream, STATS_PREV_NONE or STATS_PREV_HISTORY.  Returns the number of bytes."""
        arr = (_lib.StatsItem * max(len(items), 1))()
        for a, it in zip(arr, items):
            a.stream, a.frame, a.prev_frame = (int(v) for v in it)
        n = ctypes.c_size_t(0)
        check(self._L.h264mi_items_stats_device(self._h, ctypes.byref(stats_spec(cell, planes, thresh)), arr, len(items), dst_ptr, cap, ctypes.byref(n)))
        return n.value

    def frame_stats(self, stream=-1, cell=0, planes=(), thresh=0, items=None, history=False):
        """The statistics of the frames of `stream` (-1: of all streams, stream-major) of the last executed batch, each against the frame before it in
        output order (stats_plan), or of the (stream, frame, prev_frame) `items`: one dict per item of torch views of ONE device buffer filled by one K12
        launch.  The uint64 fields of the record are int64 scalars (0-d tensors), the uint32 scalars int32 ones -- exact, by the bounds of the contract
        --, "hist_y" is int32[256], and each selected plane ("cell_sum", "cell_sad") is int32[gh, gw].  Synchronises like side_info."""
        import torch
        bits = stats_planes(planes)
        if items is not None and history:
            raise ValueError("frame_stats: history goes with the batch form; an item names STATS_PREV_HISTORY itself")
        todo = [tuple(int(v) for v in it) for it in items] if items is not None else self.stats_plan(stream, history)
        sizes = []
        for s, f, _ in todo:
            fi = self.frame_info(s, f)
            sizes.append(self.stats_size(fi.width, fi.height, cell, bits, thresh))
        total = sum(n for _, _, n in sizes)
        out = torch.empty(max(total, 16) // 8, dtype=torch.int64, device="cuda:%d" % self.device)  # (torch allocations are at least 16-byte aligned)
        if total:
            torch.cuda.current_stream(out.device).synchronize()  # whatever still uses a recycled block has finished before K12 writes it
            if items is not None:
                got = self.stats_items(out.data_ptr(), total, todo, cell, bits, thresh)
            else:
                got = self.stats_batch(out.data_ptr(), total, stream, cell, bits, thresh, history)
            assert got == total
            self.sync()
        as32 = out.view(torch.int32)
        res, at = [], 0
        for gw, gh, n in sizes:
            q, d = at // 8, at // 4
            rec = {name: out[q + i] for i, name in enumerate(STATS_U64)}
            rec.update({name: as32[d + 16 + i] for i, name in enumerate(STATS_U32)})
            rec["hist_y"] = as32[d + 24:d + 280]
            for k, name in enumerate(pn for b, pn in enumerate(STATS_PLANE_NAMES) if bits >> b & 1):
                rec[name] = as32[d + 280 + k * gw * gh:d + 280 + (k + 1) * gw * gh].view(gh, gw)
            res.append(rec)
            at += n
        return res

    jpeg_size = staticmethod(jpeg_size)  # (header_bytes, bound_bytes): the module's function, also by the decoder's name

    def jpeg_items(self, dst_ptr, cap, slot_bytes, items, quality=90, range="auto", restart_mcus=0):
        """K13 over a list of (stream, frame) items of the last executed batch ("JPEG snapshots" of include/h264mi.h): 16-byte results (bytes, status, w,
        h), rounded up to 256 bytes, then a slot of slot_bytes per item with the item's file at its start, in the DEVICE buffer at dst_ptr (16-byte
        aligned).  Returns the number of bytes of the destination."""
        arr = (_lib.JpegItem * max(len(items), 1))()
        for a, it in zip(arr, items):
            a.stream, a.frame = (int(v) for v in it)
        n = ctypes.c_size_t(0)
        check(self._L.h264mi_items_jpeg_device(self._h, ctypes.byref(jpeg_spec(quality, range, restart_mcus)), arr, len(items), slot_bytes, dst_ptr, cap, ctypes.byref(n)))
        return n.value

    def jpeg_batch(self, dst_ptr, cap, slot_bytes, stream=-1, quality=90, range="auto", restart_mcus=0):
        """K13 for every frame of the last executed batch (of one stream, or of all streams, stream-major): jpeg_items' contract."""
        n = ctypes.c_size_t(0)
        check(self._L.h264mi_batch_jpeg_device(self._h, stream, ctypes.byref(jpeg_spec(quality, range, restart_mcus)), slot_bytes, dst_ptr, cap, ctypes.byref(n)))
        return n.value

    def jpeg_i420(self, dst_ptr, cap, slot_bytes, src_ptr, w, h, n, mono=False, quality=90, range="keep", restart_mcus=0):
        """K13 for n caller-held tight I420 frames of one size at src_ptr (DEVICE memory, back to back): jpeg_items' contract; "auto" is refused."""
        got = ctypes.c_size_t(0)
        check(self._L.h264mi_i420_jpeg_device(self._h, ctypes.byref(jpeg_spec(quality, range, restart_mcus)), src_ptr, int(w), int(h), int(bool(mono)), int(n), slot_bytes,
                                              dst_ptr, cap, ctypes.byref(got)))
        return got.value

    def _jpeg_files(self, n, slot_bytes, launch):
        """launch(indices, dst_ptr, cap, slot_bytes) encodes the items `indices` of n; items reported JPEG_TRUNCATED are encoded once more, with the size
        they asked for.  Returns the files as bytes, in item order.  Synchronises like side_info."""
        import torch
        files, todo = [None] * n, list(range(n))
        for _ in range(2):
            if not todo:
                break
            head = (16 * len(todo) + 255) & ~255
            out = torch.empty(head + len(todo) * slot_bytes, dtype=torch.uint8, device="cuda:%d" % self.device)
            torch.cuda.current_stream(out.device).synchronize()  # whatever still uses a recycled block has finished before K13 writes it
            got = launch(todo, out.data_ptr(), out.numel(), slot_bytes)
            assert got == out.numel()
            self.sync()
            res = out[:16 * len(todo)].cpu().numpy().view(np.uint32).reshape(-1, 4)
            again, need = [], 0
            for k, i in enumerate(todo):
                if res[k, 1] == 0:
                    files[i] = out[head + k * slot_bytes:head + k * slot_bytes + int(res[k, 0])].cpu().numpy().tobytes()
                else:
                    again.append(i)
                    need = max(need, int(res[k, 0]))
            todo, slot_bytes = again, (need + 15) & ~15
        assert not todo, "an item was truncated in a slot of the size it asked for"
        return files

    def i420_jpeg(self, tensor, w, h, mono=False, quality=90, range="keep", restart_mcus=0, slot_bytes=None):
        """The JPEG files (a list of bytes) of caller-held tight I420 frames of size w x h: `tensor` is a contiguous uint8 tensor on the decoder's device,
        [n, i420_size(w, h)] (for mono the luma is read and the rest ignored).  frames_tensor(..., fmt="i420", size=...) makes such tensors.  The
        default slot is the header plus w * h / 2 bytes; an item that does not fit is encoded once more with the size it asked for."""
        import torch
        assert tensor.dtype == torch.uint8 and tensor.is_contiguous() and tensor.dim() == 2 and tensor.shape[1] == self.i420_size(w, h)
        if slot_bytes is None:
            slot_bytes = (jpeg_size(w, h, mono, quality, range, restart_mcus)[0] + w * h // 2 + 15) & ~15
        stride = tensor.shape[1]
        torch.cuda.current_stream(tensor.device).synchronize()  # the frames are complete before K13 reads them on the decoder's stream

        def launch(idx, dst, cap, slot):
            if idx == list(builtins.range(idx[0], idx[0] + len(idx))):  # a contiguous run: one call
                return self.jpeg_i420(dst, cap, slot, tensor.data_ptr() + idx[0] * stride, w, h, len(idx), mono, quality, range, restart_mcus)
            sub = tensor[idx].contiguous()
            torch.cuda.current_stream(tensor.device).synchronize()
            launch.keep = sub
            return self.jpeg_i420(dst, cap, slot, sub.data_ptr(), w, h, len(idx), mono, quality, range, restart_mcus)
        return self._jpeg_files(tensor.shape[0], slot_bytes, launch)

    def frames_jpeg(self, stream=-1, quality=90, range="auto", restart_mcus=0, items=None, size=None, filter="area", slot_bytes=None):
        """The frames of `stream` (-1: of all streams, stream-major) of the last executed batch, or the (stream, frame) `items`, as baseline JPEG files: a
        list of bytes, encoded on the device (K13).  range "auto" expands limited-range streams to JPEG's full range and keeps full-range ones.
        size = (ow, oh) scales every frame first (K8 to I420, `filter` "area" or "bilinear") and encodes the scaled frames as 4:2:0 -- thumbnails.  The
        default slot is the header plus w * h / 2 bytes of the largest frame; an item that does not fit is encoded once more with the size it asked
        for."""
        if items is None:
            items = [(s, f) for s in (builtins.range(self.max_streams) if stream < 0 else (stream,)) for f in builtins.range(self.frame_count(s))]
        items = [(int(s), int(f)) for s, f in items]
        if not items:
            return []
        if size is not None:
            import torch
            ow, oh = int(size[0]), int(size[1])
            one = self.i420_size(ow, oh)
            t = torch.empty((len(items), one), dtype=torch.uint8, device="cuda:%d" % self.device)
            torch.cuda.current_stream(t.device).synchronize()
            for k, (s, f) in enumerate(items):
                self.scale_frame(s, f, t.data_ptr() + k * one, one, "i420", (ow, oh), 0, filter)
            self.sync()
            r = jpeg_spec(quality, range, restart_mcus).range
            full = [r == JPEG_RANGE_FULL or (r == JPEG_RANGE_AUTO and self.frame_colour(s, f)[1] == 0) for s, f in items]
            files = [None] * len(items)
            for want in (False, True):
                idx = [k for k, v in enumerate(full) if v == want]
                if idx:
                    sub = t if len(idx) == len(items) else t[idx].contiguous()
                    for k, data in zip(idx, self.i420_jpeg(sub, ow, oh, False, quality, "full" if want else "keep", restart_mcus, slot_bytes)):
                        files[k] = data
            return files
        if slot_bytes is None:
            infos = [self.frame_info(s, f) for s, f in items]
            slot_bytes = max((jpeg_size(fi.width, fi.height, False, quality, range, restart_mcus)[0] + fi.width * fi.height // 2 + 15) & ~15 for fi in infos)
        return self._jpeg_files(len(items), slot_bytes,
                                lambda idx, dst, cap, slot: self.jpeg_items(dst, cap, slot, [items[i] for i in idx], quality, range, restart_mcus))

    def output_order(self, stream=0):
        """Indices (decoding order) of the stream's frames of the last batch in display order: ascending PicOrderCnt per
        coded video sequence.  Only differs from range(n) for streams with B pictures."""
        n = self.frame_count(stream)
        order = (ctypes.c_int32 * max(n, 1))()
        got = ctypes.c_int32(0)
        check(self._L.h264mi_stream_output_order(self._h, stream, order, n, ctypes.byref(got)))
        return [order[i] for i in range(min(n, got.value))]

    def read_mbrecs(self, stream, frame, n_mbs):
        buf = np.zeros(n_mbs * 128, dtype=np.uint8)
        check(self._L.h264mi_frame_read_mbrecs(self._h, stream, frame, buf.ctypes.data, buf.nbytes))
        return buf.reshape(n_mbs, 128)

    def read_mbmv1(self, stream, frame, n_mbs):
        """List-1 motion vectors of a picture (int16 [n_mbs, 16, 2]; zeros for pictures without B slices)."""
        buf = np.zeros(n_mbs * 64, dtype=np.uint8)
        check(self._L.h264mi_frame_read_mbmv1(self._h, stream, frame, buf.ctypes.data, buf.nbytes))
        return buf.view(np.int16).reshape(n_mbs, 16, 2)


# ---------------------------------------------------------------------------------------------------
# Stream front-end: the reference's ByteStreamReader / handleConnection / readNalUnit
# (h264/server.go:64-172) read an endless Annex-B byte stream from a connection one byte at a time.
# Here the bytes are cut at access-unit boundaries and handed to the batched GPU decoder.

class DisplayOrder:
    """Output process for streams with B pictures: frames go in in decoding order, come out in display order.  A simplified
    C.4.5.3 "bumping": frames wait in a buffer ordered by PicOrderCnt; when more than `depth` frames wait the one with the
    smallest PicOrderCnt is released, and an IDR picture (or a picture with memory_management_control_operation 5: its
    PicOrderCnt is 0 again) releases everything before it.  `depth` must be at least the stream's number of reorder
    frames (consecutive B pictures + 1 for a B pyramid level); the SPS's max_num_ref_frames is always enough.
    (The reference has no output process: h264/server.go:113-166 stops at the parsed slice.)"""

    def __init__(self, depth=4):
        self.depth = depth
        self._wait = []  # (PicOrderCnt, arrival number, frame)
        self._n = 0

    def push(self, frame, pic_order_cnt, new_sequence=False):
        """Returns the frames that can be shown now, in display order."""
        out = []
        if new_sequence:
            out = self.flush()
        self._wait.append((pic_order_cnt, self._n, frame))
        self._n += 1
        self._wait.sort(key=lambda t: t[:2])
        while len(self._wait) > self.depth:
            out.append(self._wait.pop(0)[2])
        return out

    def flush(self):
        out = [t[2] for t in self._wait]
        self._wait = []
        return out


class AccessUnitSplitter:
    """Incremental Annex-B splitter: feed() arbitrary byte chunks, get back byte strings that end on an
    access-unit boundary (7.4.1.2.3/4): a new access unit starts at an access unit delimiter, at an SPS / PPS / SEI that follows
    a slice, or at the first slice of a new picture.  That last test is the decoder's own (h264mi_slice_starts_picture on the
    parsed slice headers, plus "a slice starts where a slice of this picture already started"): with slice groups or arbitrary
    slice order the slice of macroblock 0 is not the first of its picture, so `first_mb_in_slice == 0` -- what this class used
    to look at, and still does for slices whose parameter sets it has not seen -- would cut such pictures in the middle.
    3- and 4-byte start codes are accepted (Annex B.1); the tail that may still grow is held back until flush()."""

    def __init__(self, max_units_per_chunk=30):
        self._buf = bytearray()
        self._max = max(1, int(max_units_per_chunk))
        self._sps, self._pps = {}, {}  # parameter sets in force at the START of the buffer (those inside it are applied while scanning)

    @staticmethod
    def _nal_starts(buf):
        """offsets of the first start-code byte of every NAL unit"""
        out, i, n = [], 0, len(buf)
        while True:
            j = buf.find(b"\x00\x00\x01", i)
            if j < 0:
                return out
            out.append(j - 1 if j > 0 and buf[j - 1] == 0 else j)
            i = j + 3

    @staticmethod
    def _parameter_set(nal, sps, pps):
        """apply an SPS / PPS NAL (bytes from its header byte on) to the tables; unparsable ones are ignored"""
        try:
            nu = NewNalUnit(bytes(nal))
            if nu.Type == 7:
                s = NewSPS(nu.RBSP())
                sps[s.ID] = s
            elif nu.Type == 8 and len(nu.RBSP()) > 1:
                br = nu.RBSP()
                # seq_parameter_set_id is the second ue(v): parse against every known SPS until one accepts it (ids are small)
                for cand in list(sps.values()):
                    try:
                        q = NewPPS(cand, br)
                        if q.SPSID == cand.ID:
                            pps[q.ID] = q
                            break
                    except H264MIError:
                        continue
        except H264MIError:
            pass

    @staticmethod
    def _slice_header(nal, sps, pps):
        """(first_mb_in_slice, header, sps) of a slice NAL, or None if its parameter sets are unknown / it does not parse"""
        for n in (min(len(nal), 768), len(nal)):  # the header nearly always ends within the first bytes
            try:
                nu = NewNalUnit(bytes(nal[:n]))
                rb = nu.RBSP()
                # pic_parameter_set_id: third ue(v) of the header -- let every known PPS try (a stream rarely has more than one)
                for q in list(pps.values()):
                    sp = sps.get(q.SPSID)
                    if sp is None:
                        continue
                    try:
                        h = NewSliceContext(VideoStream(sp, q), nu, rb).Slice.Header
                        if h.PPSID == q.ID:
                            return h.FirstMbInSlice, h, sp
                    except H264MIError:
                        continue
            except H264MIError:
                pass
        return None

    def _boundaries(self, final):
        """offsets at which a new access unit starts (excluding 0), in order"""
        buf = self._buf
        starts = self._nal_starts(buf)
        sps, pps = dict(self._sps), dict(self._pps)
        cuts, seen_vcl = [], False
        first_hdr, first_mbs = None, set()
        L = _lib.load()
        for k, off in enumerate(starts):
            j = buf.find(b"\x00\x00\x01", off) + 3
            if j >= len(buf):
                break  # header byte not here yet
            end = starts[k + 1] if k + 1 < len(starts) else len(buf)
            complete = k + 1 < len(starts) or final
            t = buf[j] & 31
            if t in (1, 5):
                if not complete:
                    break  # the slice header may still be arriving
                parsed = self._slice_header(buf[j:end], sps, pps)
                if parsed is None:  # parameter sets unknown: the old rule
                    new_pic = j + 1 < len(buf) and (buf[j + 1] & 0x80) != 0
                    first_mb, hdr = (0 if new_pic else -1), None
                else:
                    first_mb, hdr, sp = parsed
                    new_pic = first_mb in first_mbs or (first_hdr is not None and L.h264mi_slice_starts_picture(ctypes.byref(sp._c), ctypes.byref(first_hdr._c), ctypes.byref(hdr._c)) == 1)
                if seen_vcl and new_pic:
                    cuts.append(off)
                    first_hdr, first_mbs = None, set()
                if first_hdr is None:
                    first_hdr = hdr
                first_mbs.add(first_mb)
                seen_vcl = True
            elif t in (6, 7, 8, 9):
                if seen_vcl:
                    cuts.append(off)
                    seen_vcl, first_hdr, first_mbs = False, None, set()
                if t in (7, 8) and complete:
                    self._parameter_set(buf[j:end], sps, pps)
            elif t in (10, 11) and seen_vcl:  # end of sequence / stream belong to the access unit they follow
                nxt = starts[k + 1] if k + 1 < len(starts) else None
                if nxt is not None:
                    cuts.append(nxt)
                    seen_vcl, first_hdr, first_mbs = False, None, set()
        # de-duplicate while keeping order
        out = []
        for c in cuts:
            if c > 0 and (not out or c > out[-1]):
                out.append(c)
        return out

    def feed(self, data: bytes):
        """Append bytes; returns a list of chunks, each holding whole access units (at most max_units_per_chunk)."""
        self._buf += data
        return self._emit(False)

    def flush(self):
        """End of stream: everything that is left is the last access unit(s)."""
        return self._emit(True)

    def _emit(self, final):
        cuts = self._boundaries(final)
        if final:
            cuts = cuts + [len(self._buf)]
        chunks, prev, k = [], 0, 0
        while k < len(cuts):
            take = min(self._max, len(cuts) - k)
            end = cuts[k + take - 1]
            if end > prev:
                chunks.append(bytes(self._buf[prev:end]))
            prev, k = end, k + take
        if prev:  # the parameter sets inside what leaves are in force for what stays
            head = self._buf[:prev]
            st = self._nal_starts(head)
            for k, off in enumerate(st):
                j = head.find(b"\x00\x00\x01", off) + 3
                if j < len(head) and (head[j] & 31) in (7, 8):
                    self._parameter_set(head[j:st[k + 1] if k + 1 < len(st) else len(head)], self._sps, self._pps)
        del self._buf[:prev]
        return chunks


END_OF_STREAM = b"\x00\x00\x00\x01\x0b"  # nal_unit_type 11: tells the decoder that nothing follows -- a first field still waiting for its second one goes out as it is


class H264Reader:
    """Mirror of the reference's H264Reader + handleConnection loop (h264/server.go:113-166): reads a connection
    (anything with recv() or read()), cuts the byte stream at access units and decodes them on the GPU.
    `on_frames(frames)` receives uint8[n, width*height*3/2] arrays (cropped I420) in decoding order, or -- with
    display_order=N -- in display order through a DisplayOrder buffer of depth N (streams with B pictures)."""

    def __init__(self, connection, decoder=None, on_frames=None, max_width=1920, max_height=1088, frames_per_batch=30, read_size=1 << 16, display_order=0,
                 conceal_errors=False, random_access=False):
        self.Stream = connection
        self.frames_per_batch = frames_per_batch
        self.decoder = decoder or Decoder(max_streams=1, max_width=(max_width + 15) // 16 * 16, max_height=(max_height + 15) // 16 * 16,
                                          max_frames_per_batch=_frames_with_headroom(frames_per_batch, conceal_errors), max_slices_per_frame=16,
                                          conceal_errors=conceal_errors)
        if random_access:  # a connection that starts in the middle of a stream: decode from its first recovery point on (Decoder.set_random_access)
            self.decoder.set_random_access(random_access)
        self.on_frames = on_frames
        self.read_size = read_size
        self.splitter = AccessUnitSplitter(frames_per_batch)
        self.n_frames = 0
        self._dims = (0, 0)
        self._reorder = DisplayOrder(display_order) if display_order else None

    def _read(self):
        s = self.Stream
        return s.recv(self.read_size) if hasattr(s, "recv") else s.read(self.read_size)

    def _decode(self, chunks):
        for c in chunks:
            self.decoder.decode([c])
            n = self.decoder.frame_count(0)
            if n:
                frames = [self.decoder.read_frame(0, f, crop=True)[:self._size()] for f in range(n)]
                self.n_frames += n
                if self._reorder:
                    shown = []
                    for f in range(n):
                        fi = self.decoder.frame_info(0, f)
                        shown += self._reorder.push(frames[f], fi.pic_order_cnt, bool(fi.new_sequence))
                    frames = shown
                if self.on_frames and len(frames):
                    self.on_frames(np.stack(frames))

    def _size(self):
        info = self.decoder.info
        if info.width and info.height:
            self._dims = (info.width, info.height)
        return Decoder.i420_size(*self._dims)

    def run(self):
        """Read until the peer closes the connection; returns the number of decoded frames."""
        while True:
            data = self._read()
            if not data:
                break
            self._decode(self.splitter.feed(data))
        self._decode(self.splitter.flush() + [END_OF_STREAM])
        if self._reorder:
            rest = self._reorder.flush()
            if self.on_frames and rest:
                self.on_frames(np.stack(rest))
        return self.n_frames


def handleConnection(connection, **kw):
    """h264/server.go:113 -- decode everything arriving on `connection`; returns the frame count."""
    return H264Reader(connection, **kw).run()


def ByteStreamReader(connection, **kw):
    """h264/server.go:168 -- same, and closes the connection afterwards."""
    try:
        return handleConnection(connection, **kw)
    finally:
        if hasattr(connection, "close"):
            connection.close()


class BatchServer:
    """Several connections decoded side by side: every connection owns one stream slot of ONE batched Decoder, and each
    tick hands one chunk (whole access units) per connection that has one to a single h264mi_decode_batch call -- the
    batch scheduler the reference's per-connection goroutine (main.go:12-21) lacks.  `on_frames(slot, frames)` receives
    the cropped I420 frames of a connection in decoding order; `on_close(slot, n_frames)` when its peer is done."""

    def __init__(self, max_connections=8, max_width=1920, max_height=1088, frames_per_batch=30, on_frames=None, on_close=None, read_size=1 << 16, conceal_errors=False,
                 random_access=False):
        self.decoder = Decoder(max_streams=max_connections, max_width=(max_width + 15) // 16 * 16, max_height=(max_height + 15) // 16 * 16,
                               max_frames_per_batch=_frames_with_headroom(frames_per_batch, conceal_errors), max_slices_per_frame=16, conceal_errors=conceal_errors)
        self.decoder.set_isolation(True)  # one bad client must not take the other connections' chunks down with it
        if random_access:  # clients may connect in the middle of a stream, and a stream that lost a picture comes back at its next recovery point
            self.decoder.set_random_access(random_access)
        self.errors = [0] * max_connections
        self.n = max_connections
        self.frames_per_batch = frames_per_batch
        self.on_frames, self.on_close, self.read_size = on_frames, on_close, read_size
        self.conn = [None] * self.n       # socket-like object per slot
        self.split = [None] * self.n
        self.queue = [[] for _ in range(self.n)]  # chunks waiting to be decoded
        self.eof = [False] * self.n
        self.count = [0] * self.n
        self.dims = [(0, 0)] * self.n

    def add(self, connection):
        """Attach a connection to a free slot; returns the slot or -1 when the server is full."""
        for i in range(self.n):
            if self.conn[i] is None:
                self.conn[i], self.split[i], self.queue[i], self.eof[i], self.count[i] = connection, AccessUnitSplitter(self.frames_per_batch), [], False, 0
                self.dims[i], self.errors[i] = (0, 0), 0
                self.decoder.reset_stream(i)  # nothing of the slot's previous client (parameter sets, reference pictures) survives
                if hasattr(connection, "setblocking"):
                    connection.setblocking(False)
                return i
        return -1

    def _pump(self, i):
        """Read what the connection has; returns True if anything arrived or it closed."""
        c = self.conn[i]
        try:
            data = c.recv(self.read_size) if hasattr(c, "recv") else c.read(self.read_size)
        except (BlockingIOError, InterruptedError):
            return False
        if data:
            self.queue[i] += self.split[i].feed(data)
        else:
            self.queue[i] += self.split[i].flush() + [END_OF_STREAM]  # (a lone first field at the end of the connection still goes out)
            self.eof[i] = True
        return True

    def tick(self):
        """One scheduling step: read every connection, decode one chunk per connection in one batch.  Returns the number
        of frames decoded."""
        for i in range(self.n):
            if self.conn[i] is not None and not self.eof[i]:
                self._pump(i)
        batch = [self.queue[i].pop(0) if (self.conn[i] is not None and self.queue[i]) else b"" for i in range(self.n)]
        total = 0
        if any(batch):
            self.decoder.decode(batch)
            for i in range(self.n):
                if not batch[i]:
                    continue
                st = self.decoder.stream_status(i)
                if st != 0:  # this connection's chunk was malformed / out of scope: close it, the others go on
                    self.errors[i] = st
                    self.queue[i] = []
                    self.eof[i] = True
                    continue
                k = self.decoder.frame_count(i)
                if not k:
                    continue
                frames = [self.decoder.read_frame_tight(i, f, crop=True) for f in range(k)]
                fi = self.decoder.frame_info(i, k - 1)
                self.dims[i] = (fi.width, fi.height)
                # frames of one geometry go out together (a chunk may span a resolution change)
                start = 0
                for f in range(1, k + 1):
                    if f == k or len(frames[f]) != len(frames[start]):
                        if self.on_frames:
                            self.on_frames(i, np.stack(frames[start:f]))
                        start = f
                self.count[i] += k
                total += k
        for i in range(self.n):
            if self.conn[i] is not None and self.eof[i] and not self.queue[i]:
                c, n = self.conn[i], self.count[i]
                self.conn[i] = None
                if hasattr(c, "close"):
                    c.close()
                if self.on_close:
                    self.on_close(i, n)
        return total

    def active(self):
        return sum(c is not None for c in self.conn)

    def run(self, idle_sleep=0.001):
        """Serve until every attached connection has closed."""
        import time
        while self.active():
            if not self.tick():
                time.sleep(idle_sleep)
        return list(self.count)

