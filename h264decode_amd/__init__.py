"""h264decode_amd -- MI355X-native H.264 Annex-B decode path (HIP, gfx950) behind the API names of
the Go package `h264` of mrmod/h264decode.

The pixel path exists only on the GPU: importing works anywhere (header parsing is host code), but
creating a Decoder without a HIP device or without the built libh264mi.so raises."""
from ._lib import H264MIError, build, lib, load, load_hooks  # noqa: F401
from .h264 import (  # noqa: F401
    NALU_TYPE_NAMES, PPS, SPS, Decoder, NalUnit, NewNalUnit, NewPPS, NewSPS, NewSliceContext, SliceContext, SliceHeader,
    VideoStream, read_nal_units, MapUnitToSliceGroupMap, MbToSliceGroupMap, nextMbAddress, AccessUnitSplitter, DisplayOrder, H264Reader, handleConnection, ByteStreamReader, BatchServer,
    CONCEAL_SLICES, CONCEAL_PICTURES, CONCEAL_FIELDS, CONCEAL_IDR, CONCEAL_LONE_FIELDS, CONCEAL_MAX_GAP, RA_OFF, RA_RECOVERY_POINT,
    FMT_I420, FMT_NV12, FMT_RGB24, FMT_RGBP, CSC_AUTO, CSC_BT601, CSC_BT709, CSC_FULL_RANGE, CSC_CHROMA_BILINEAR,
    SCALE_BILINEAR, SCALE_AREA, scale_taps,
    DT_U8, DT_F16, DT_BF16, DT_F32, FIT_STRETCH, FIT_LETTERBOX, TENSOR_BGR, fit_rect, tensor_spec,
    DEINT_FIELD, DEINT_BLEND, DEINT_EDGE, DEINT_PARITY_FIRST, STREAM_DERIVED, deint_rows,
    DEINT_PREV_NONE, DEINT_PREV_HISTORY, DEINT_HISTORY, deint_motion_pixel,
    STATS_CELL_SUM, STATS_CELL_SAD, STATS_PLANE_NAMES, STATS_PREV_NONE, STATS_PREV_HISTORY, STATS_HISTORY, STATS_U64, STATS_U32, stats_planes, stats_spec,
    JPEG_RANGE_AUTO, JPEG_RANGE_KEEP, JPEG_RANGE_FULL, JPEG_TRUNCATED, jpeg_spec, jpeg_size, jpeg_quant_table, jpeg_block,
    SIDE_NAMES, SIDE_ALL, side_planes, MB_NONE, MB_I4x4, MB_I8x8, MB_I16x16, MB_IPCM, MB_P16x16, MB_P16x8, MB_P8x16, MB_P8x8, MB_PSKIP, MB_B, MB_BDIRECT, MB_BSKIP)
from .mbtype import (  # noqa: F401
    MB_TYPE_INFERRED, ISliceMbType, SISliceMbType, PSliceMbType, BSliceMbType, MbTypeName, MbPartPredMode, NumMbPart, PicWidthInMbs,
    PicHeightInMapUnits, PicSizeInMapUnits, FrameHeightInMbs, PicHeightInMbs, PicSizeInMbs, SubWidthC, SubHeightC, MbWidthC, MbHeightC,
    MbaffFrameFlag, CodedBlockPatternLuma, CodedBlockPatternChroma, Clip3, Clip1y, Clipc, SliceQPy, PreCtxState, SliceData, NewSliceData, MbPred)
