// h264decode_amd/csrc/k_entropy_m.hip -- the Main build of the I/P slice_data() kernel: k_entropy.hip compiled with the entropy coding
// mode as the constant "CABAC" (as k_entropy_c.hip) and, on top of that, transform_8x8_mode = 0 and 4:2:0 as constants: no
// transform_size_8x8_flag, no Intra8x8 modes, no ctxBlockCat 5, no monochrome arms.  A separate kernel: level 0 of a batch uses it when
// every one of its slices is CABAC-coded, no picture has slice groups, and no picture of the batch has the 8x8 transform switched on or is
// monochrome (mi_entropy_kernel_choice); one such picture sends the launch to k_entropy_c.
#define MI_ENT_CABAC 1
#define MI_ENT_MAIN 1
#include "k_entropy.hip"
