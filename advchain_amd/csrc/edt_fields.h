// The squared-distance fields of csrc/edt.hip for the other translation units (seg_surface.hip): the passes of the transform
// without its finish.  Host code only; the kernels stay in edt.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace advchain {

// Words of `fields` for `entries` label maps of K classes, or -1: ADVCHAIN_ERR_ARG / ADVCHAIN_ERR_UNSUPPORTED shapes (the
// limits of advchain_signed_maps: include/advchain_hip.h) and sizes that do not fit.
int64_t edt_label_fields_words(int64_t entries, int64_t K, int ndim, const int64_t* dims);

// labels (entries, dims) int64 -> fields (entries, K, dims): per voxel the squared distance to the nearest member of class k of
// its entry, or the sentinel where the class is absent.  sampling NULL: int32 squares (exact), sentinel 2^30; otherwise ndim
// host floats and fp32 squares, sentinel 1e30.  A label outside [0, K) belongs to no class.  Enqueues on `st`; returns
// ADVCHAIN_OK or an error code with advchain_last_error() set (`what` prefixes the message).
int edt_label_fields(const int64_t* labels, const float* sampling, void* fields, int64_t entries, int64_t K, int ndim,
                     const int64_t* dims, const char* what, hipStream_t st);

}  // namespace advchain
