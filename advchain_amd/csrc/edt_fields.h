// The squared-distance fields of csrc/edt.hip for the other translation units (seg_surface.hip, seg_morph.hip): the passes of the
// transform without its finish.  Host code only; the kernels stay in edt.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace advchain {

// "no seed": the value of a field word that no seed has reached (int32 squares with unit spacing, fp32 with a sampling)
constexpr int kEdtFieldInf = 1 << 30;
constexpr float kEdtFieldInfF = 1.0e30f;

// Words of `fields` for `entries` label maps of K classes, or -1: ADVCHAIN_ERR_ARG / ADVCHAIN_ERR_UNSUPPORTED shapes (the
// limits of advchain_signed_maps: include/advchain_hip.h) and sizes that do not fit.
int64_t edt_label_fields_words(int64_t entries, int64_t K, int ndim, const int64_t* dims);

// labels (entries, dims) int64 -> fields (entries, K, dims): per voxel the squared distance to the nearest member of class k of
// its entry, or the sentinel where the class is absent.  sampling NULL: int32 squares (exact), sentinel 2^30; otherwise ndim
// host floats and fp32 squares, sentinel 1e30.  A label outside [0, K) belongs to no class.  Enqueues on `st`; returns
// ADVCHAIN_OK or an error code with advchain_last_error() set (`what` prefixes the message).
int edt_label_fields(const int64_t* labels, const float* sampling, void* fields, int64_t entries, int64_t K, int ndim,
                     const int64_t* dims, const char* what, hipStream_t st);

// The checks of edt_label_fields without a launch: ADVCHAIN_OK with d = (D, H, W) (D = 1 in 2D) and the spacing s of those axes
// (1 without a sampling), or the error code it would return, with the same message.
int edt_fields_check(const float* sampling, int64_t entries, int64_t K, int ndim, const int64_t* dims, const char* what,
                     int64_t (&d)[3], float (&s)[3]);

// mask (entries, dims) 8-bit -> fields (entries, dims): per voxel the squared distance to the nearest NONZERO voxel of its entry, or
// the sentinel where the entry has none.  Otherwise as edt_label_fields with K = 1 (words: edt_label_fields_words(entries, 1, ..)).
int edt_mask_fields(const unsigned char* mask, const float* sampling, void* fields, int64_t entries, int ndim, const int64_t* dims,
                    const char* what, hipStream_t st);

}  // namespace advchain
