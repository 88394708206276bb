// h264decode_amd/csrc/k_entropy_c.hip -- the CABAC-only build of the I/P slice_data() kernel: k_entropy.hip compiled with the entropy
// coding mode as the constant "CABAC" (Main / High profile streams) instead of a per-slice value, and without the CAVLC parser and its
// tables.  A separate kernel: level 0 of a batch uses it when every one of its slices is CABAC-coded and no picture has slice groups
// (mi_entropy_kernel_choice); one CAVLC slice in the launch sends it to k_entropy.
#define MI_ENT_CABAC 1
#include "k_entropy.hip"
