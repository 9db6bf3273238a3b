// fedagg_internal.h -- what libfedagg's translation units share beyond the C ABI of
// include/fedagg.h.  Everything here is defined in fedagg.hip.
#pragma once

#include "fedagg.h"

#define FA_BLOCK 256  // threads per workgroup of the kernels

namespace fedagg_internal {

// The calling thread's fedagg_last_error() text.
void set_error(const char* msg);
// Sets the error text (fmt takes one %lld, given b) and returns code.
int fail(int code, const char* fmt, long long b = 0);
// FEDAGG_OK, or FEDAGG_EHIP with "<what>: <hip error>" as the text when the last launch failed.
int check_launch(const char* what);
// The "flat_vec" knob of fedagg_tune: 16-B accesses in the client flat ops.
int flat_vec();
// The "fuse_pairwise" knob: numel == 1 elements patched inside the bucket launch.
int fuse_pairwise();
// Workgroups of FA_BLOCK threads for `work` threads, under the "grid_cap" knob.
unsigned launch_grid(uint64_t work);

}  // namespace fedagg_internal
