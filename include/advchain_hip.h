/* advchain_hip.h -- C ABI of libadvchain_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the ONE hot path of cherise215/advchain: the adversarial-augmentation
 * inner loop (ComposeAdversarialTransformSolver over AdvNoise / AdvBias / AdvMorph / AdvAffine).
 * The reference has no native layer of its own: its arithmetic is a set of PyTorch ATen call
 * sites.  Each entry point below replaces one (or a fused run) of those call sites; the
 * "replaces" line cites the reference file:line (paths relative to the upstream repo root).
 *
 * Contract (all entry points)
 *   - extern "C", plain pointers and sizes, no torch types.  Pointers are DEVICE pointers to
 *     contiguous fp32 (int32 for index tables) owned by the caller; nothing is allocated or
 *     freed inside; outputs / workspaces are caller-allocated.
 *   - layout: channels-first (N, C, S0, S1[, S2]); `ndim` = 2 or 3 spatial dims, `dims` has
 *     `ndim` entries in tensor order (slowest first).  Sampling grids are PLANAR (N, ndim, ...)
 *     with channel 0 = x <-> last spatial dim, 1 = y, 2 = z (F.grid_sample convention).  The sampler entry
 *     points (grid_sample, compose_self, expo_chain, affine_warp) take volumes of at least two voxels.
 *   - align_corners=True everywhere (the reference never uses False for samplers).
 *   - `stream` is a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); kernels are
 *     enqueued asynchronously on it; the call never synchronises.
 *   - returns 0 on success, <0 on error (ADVCHAIN_ERR_*); advchain_last_error() gives the
 *     message (thread-local).  No exceptions cross the ABI.  Thread-safe for distinct
 *     streams/buffers.
 *   - backward entry points whose targets are scatter destinations (grad_in / grad_phi) require
 *     the caller to zero them first; they accumulate with hardware fp32 atomics.
 */
#ifndef ADVCHAIN_HIP_H_
#define ADVCHAIN_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADVCHAIN_INTERP_LINEAR 0  /* 'bilinear' (4-D) / trilinear (5-D) */
#define ADVCHAIN_INTERP_NEAREST 1
#define ADVCHAIN_INTERP_BICUBIC 2  /* 2D only; its own entry points (advchain_grid_sample_bicubic2d_*) */
#define ADVCHAIN_PAD_ZEROS 0
#define ADVCHAIN_PAD_BORDER 1
#define ADVCHAIN_PAD_REFLECTION 2

int advchain_version(void);
const char* advchain_last_error(void);

/* ---- deterministic mode (round 6) ---------------------------------------------------------
 * replaces: nothing the reference writes down -- its CPU path (the parity target) is deterministic by construction, and
 *           on a GPU it inherits torch.use_deterministic_algorithms(), under which grid_sampler_{2,3}d_backward
 *           (reached from adv_morph.py:546-557 through autograd) raises for want of a deterministic kernel.  Here the one
 *           formulation of the C <= 4 routes whose bits depend on arrival order -- the source-tiled window scatter (2D
 *           image warps above 16 px, squarings above 32 px; 3D above 4 voxels), which flushes its LDS windows with float
 *           atomics -- gets a bit-reproducible twin: the tiles add 64-bit fixed point (2^40 / max|grad_out| of the batch
 *           entry) into an int64 image of grad_in inside the caller's workspace and one more pass converts it.  The
 *           general float-atomic kernels (warps of more than four channels, nearest, size-changing; the affine scatter
 *           of more than eight channels) and the bicubic backward have twins of the same kind as entries of their own --
 *           advchain_grid_sample_bwd_det, advchain_affine_warp_bwd_det, advchain_grid_sample_bicubic2d_bwd_det -- which the
 *           Python layer calls when the switch is on.  Every other backward formulation (gather forms, owner-computes
 *           scatters, affine tiles) is deterministic already.  Two VALUES are covered the same way, by entries the Python
 *           layer calls when the switch is on: the consistency loss (the *_fwd_ord entries + advchain_consistency_finish_ord:
 *           one partial per workgroup, added in a fixed order, instead of float atomics into 64 slots) and the norm behind the
 *           3D step count (advchain_tp_interp_sumsq_ordered).  The step count DOES depend on that norm -- a last-bit
 *           difference at a power-of-two threshold changes the number of squarings and with it every result of the call --
 *           so bit-reproducible 3D morph chains need the ordered norm.  The supervised losses (seg_loss.hip) always reduce
 *           in a fixed order.
 * PROCESS-WIDE switch, read when a backward entry is called and by advchain_scatter_workspace (which then returns the larger
 * size: allocate workspaces AFTER setting the mode; a workspace sized in the other mode must not be reused).  Not covered
 * (still float atomics): the overflow list of the LDS-tiled scatter (reflection padding, 3-channel image warps, calls without
 * a displacement bound), nearest-neighbour / size-changing backward THROUGH advchain_grid_sample_bwd ITSELF (call
 * advchain_grid_sample_bwd_det), the bicubic backward THROUGH advchain_grid_sample_bicubic2d_bwd ITSELF (call its _det
 * twin), and affine samples flagged as degenerate by the gather form (C <= 8).  The switch is per process, not per call.  */
void advchain_set_deterministic(int on);
int advchain_get_deterministic(void);

/* ---- dense-field warp ------------------------------------------------------------------
 * replaces: F.grid_sample(data, grid.permute(..), mode, padding_mode, align_corners=True)
 *           advchain/augmentor/adv_morph.py:546-557 (AdvMorph.transform), and the final
 *           torch.clamp(dxy,-1,1) of adv_morph.py:304-305,490 when clamp_grid != 0 (the
 *           clamp and its sub-gradient mask are applied to the grid on load).
 * in (N,C,in_dims), grid (N,ndim,out_dims) planar, out (N,C,out_dims).                      */
/* clamp_grid: bit 0 = clamp the grid to [-1, 1] on load; bits 8..15 (optional) = the caller's estimate of the grid's
 * displacement |position - own voxel| in voxels, rounded up, 0 = unknown -- a performance hint that selects the forward
 * kernel (z-marching below one voxel, LDS tiles above); results do not depend on it.  advchain_compose_self_fwd takes the
 * same hint in bits 8..15 of final_mode. */
int advchain_grid_sample_fwd(const float* in, const float* grid, float* out, int64_t N, int64_t C, int ndim,
                             const int64_t* in_dims, const int64_t* out_dims, int interp, int padding,
                             int clamp_grid, void* stream);
/* The call above for two tensors through ONE grid: out = warp(in) (C channels) and ride_out = warp(ride_in) (one channel,
 * (N,1,in_dims) -> (N,1,out_dims)).
 * replaces: the pair of F.grid_sample calls the reference's solver makes with one deformation -- the data warp
 *           (adv_compose_solver.py:148-176 forward / 199-219 backward -> adv_morph.py:546-557) and the warp of the all-ones
 *           validity mask through the same transform (adv_compose_solver.py:262-268, 321-325).  2D: one launch (the taps of
 *           a sample are built once); 3D: the two launches of advchain_grid_sample_fwd.  Values are those of two separate
 *           calls, bit for bit.  flags bit 0: ride_out = (warp(ride_in) != 0) as 0 / 1 (the `masks[masks != 0] = 1` of
 *           adv_compose_solver.py:266-268 after the last warp of the round trip).                                      */
int advchain_grid_sample_fwd_ride(const float* in, const float* grid, float* out, const float* ride_in, float* ride_out,
                                  int64_t N, int64_t C, int ndim, const int64_t* in_dims, const int64_t* out_dims,
                                  int interp, int padding, int clamp_grid, int flags, void* stream);
/* replaces: autograd grid_sampler_{2,3}d_backward for the call above.
 * grad_in (N,C,in_dims) and grad_grid (N,ndim,out_dims); either may be NULL.  grad_grid is overwritten.
 * With `workspace` (int32[advchain_scatter_workspace(N,ndim,dims)]) grad_in is simply overwritten: the
 * LDS-tiled owner-computes scatter (64-bit fixed-point accumulation, deterministic) is used for linear
 * interpolation with in_dims == out_dims and C <= 4, and grad_in is zero-filled internally otherwise;
 * with workspace == NULL the global-atomic path is used and grad_in must be pre-zeroed by the caller.
 * halo > 0: an upper bound on the displacement |sampling position - own voxel| in voxels (see
 * advchain_max_displacement) -- a performance hint only: small bounds (1 in 3D, <= 4 in 2D; C in {1,4}) select the
 * gather-form adjoint (no atomics), larger ones size the tile halo; samples beyond the bound stay correct through the
 * overflow list.  Bounds above the gather form (2D: any; 3D: hints >= 2, i.e. one voxel and more) select the
 * source-tiled window scatter (float atomics between tiles: summation order, ~1e-7 relative, varies run to run).
 * 0 = default tiles.  halo < 0: |halo| is exact (guaranteed by the caller): see advchain_compose_self_bwd.  */
int64_t advchain_scatter_workspace(int64_t N, int ndim, const int64_t* dims); /* int32 elements (larger in deterministic mode) */
int advchain_grid_sample_bwd(const float* grad_out, const float* in, const float* grid, float* grad_in,
                             float* grad_grid, int32_t* workspace, int64_t N, int64_t C, int ndim,
                             const int64_t* in_dims, const int64_t* out_dims, int interp, int padding, int clamp_grid,
                             int halo, void* stream);
/* Deterministic twin of the GENERAL kernel of the call above (the one it uses for C > 4, nearest interpolation or
 * in_dims != out_dims: any C >= 1, 2D / 3D, linear / nearest, every padding, clamp_grid bit 0).
 * replaces: the same grid_sampler_{2,3}d_backward, as torch.use_deterministic_algorithms() would want it (it raises instead).
 * grad_in is accumulated with 64-bit integer atomics as fixed point, 2^bits / max|grad_out| of the batch entry with
 * bits = min(40, 62 - ceil(log2(out voxels per sample))), in an int64 image inside `det_ws`
 * (int32[advchain_det_warp_workspace(N, C, ndim, in_dims)]: 2 N C V for the image + N maxima padded to a multiple of 4;
 * 8-byte aligned; host-only size query, independent of the switch), and one more pass converts it: equal bits run to run,
 * quantum max|grad_out| / 2^bits per deposit; a NaN / inf in an entry's grad_out turns that entry's grad_in into NaN.
 * grad_in is overwritten (no pre-zeroing); grad_grid is bit for bit what advchain_grid_sample_bwd's general kernel writes.
 * Works whatever advchain_get_deterministic() says -- the switch is consulted by the Python layer, not here.  Four launches
 * (clear, maxima, scatter, convert), all kernels.                                                                    */
/* advchain_grid_sample_bwd with a staging buffer for its source-tiled window scatter: the same checks and the same routing
 * (whole-row scatter -> gather form -> window scatter -> tiles).
 * replaces: the same grid_sampler_2d_backward.  In deterministic mode the window route of advchain_grid_sample_bwd clears an
 *           int64 image of grad_in, takes a maximum of grad_out per entry, flushes its LDS windows with 64-bit integer atomics
 *           and converts the image.  With `stage_ws` (int32[advchain_window_stage_workspace(N, C, ndim, in_dims)], 16-byte
 *           aligned, not initialised) and ndim == 2 it takes the STAGED form instead: the window kernel stores every tile's
 *           window (32-bit cells at the tile's scale) and a header in a slot of its own, and a merge kernel -- one workgroup
 *           per 32 x 32 tile of grad_in -- takes the entry's maximum from the headers, sums the staged cells that cover its
 *           pixels as 64-bit fixed point in registers and stores every pixel.  Two launches, no clear, no global atomic;
 *           grad_in and grad_grid are bit for bit those of the int64 twin, for any field (the corners a tile's capped window
 *           leaves out are rebuilt by the merge kernel and rounded as the twin rounds them).
 * The staged form is taken only in deterministic mode; stage_ws == NULL, ndim == 3 or the default mode give
 * advchain_grid_sample_bwd itself.  The size query is host-only and independent of the switch: tiles * (8 + 8192) ints per
 * entry (tiles of 32 x 32 samples; 12288 for C == 4), 0 where the form does not exist (3D, C not in {1, 2, 4}), -1 for bad
 * arguments.  advchain_scatter_workspace keeps its sizes.                                                                 */
int64_t advchain_window_stage_workspace(int64_t N, int64_t C, int ndim, const int64_t* in_dims); /* int32 elements */
int advchain_grid_sample_bwd_staged(const float* grad_out, const float* in, const float* grid, float* grad_in,
                                    float* grad_grid, int32_t* workspace, int64_t N, int64_t C, int ndim,
                                    const int64_t* in_dims, const int64_t* out_dims, int interp, int padding, int clamp_grid,
                                    int halo, void* stream, int32_t* stage_ws);
/* The formulation the last advchain_grid_sample_bwd / advchain_grid_sample_bwd_staged call of THIS THREAD ended in, noted on the
 * host by the launcher (nothing on the device): tests and tools use it to show which kernel a case ran.                   */
#define ADVCHAIN_ROUTE_NONE 0
#define ADVCHAIN_ROUTE_GENERAL 1        /* the general float-atomic kernel */
#define ADVCHAIN_ROUTE_ROWS 2           /* 2D whole-row owner-computes scatter */
#define ADVCHAIN_ROUTE_GATHER 3         /* gather-form adjoint */
#define ADVCHAIN_ROUTE_MARCH 4          /* 3D owner-computes march */
#define ADVCHAIN_ROUTE_WINDOW_FLOAT 5   /* window scatter, float-atomic flush */
#define ADVCHAIN_ROUTE_WINDOW_INT64 6   /* window scatter, int64 image (deterministic mode) */
#define ADVCHAIN_ROUTE_WINDOW_STAGED 7  /* window scatter, staged windows + merge (deterministic mode, 2D) */
#define ADVCHAIN_ROUTE_TILED 8          /* LDS-tiled owner-computes scatter */
int advchain_last_bwd_route(void);
int64_t advchain_det_warp_workspace(int64_t N, int64_t C, int ndim, const int64_t* in_dims); /* int32 elements */
int advchain_grid_sample_bwd_det(const float* grad_out, const float* in, const float* grid, float* grad_in,
                                 float* grad_grid, int32_t* det_ws, int64_t N, int64_t C, int ndim,
                                 const int64_t* in_dims, const int64_t* out_dims, int interp, int padding, int clamp_grid,
                                 void* stream);

/* ---- scaling-and-squaring step ---------------------------------------------------------
 * replaces: applyComposition{2,3}D(phi, phi) = F.grid_sample(phi, phi^T, 'border',
 *           align_corners=True), adv_morph.py:179-202, called 8+ times from
 *           vectorFieldExponentiation{2,3}D adv_morph.py:132-135,165-168.
 * final_mode 1 additionally emits (sample - phi0) + identity, i.e. 'phi - grid_wh' (with the
 * in-place aliasing of adv_morph.py:111,143,176) plus '+ self.base_grid' of :474,483.
 * phi, out, phi0: (N, ndim, dims).
 * disp_out (may be NULL): ADVCHAIN_DISP_SLOTS (4096) floats, zero-initialised by the caller; the kernel
 * max-accumulates (atomically, spread over the slots) the displacement |position - own voxel| of `out` in voxels --
 * the max over the slots is the bound the backward of the NEXT squaring wants (advchain_compose_self_bwd: halo). */
#define ADVCHAIN_DISP_SLOTS 4096
int advchain_compose_self_fwd(const float* phi, float* out, const float* phi0, int64_t N, int ndim,
                              const int64_t* dims, int final_mode, float* disp_out, void* stream);
/* grad_phi receives both the value path (scatter) and the coordinate path; overwritten when a
 * `workspace` (as above) is given, otherwise it must be pre-zeroed (global-atomic path).
 * chain != 0: grad_out is the grad_phi of the previous call on the same workspace (the backward of
 * consecutive squarings).  Accepted for callers that pass it; no formulation scales by a maximum handed from one call to
 * the next any more (the LDS-tiled scatter, which did, takes its fixed-point scale -- 2^30 / max|grad_out| -- over the
 * samples each workgroup reads, tile + halo: an entry's result does not depend on the rest of the batch).
 * halo > 0: an upper bound on |displacement| of phi in voxels -- a performance hint only: samples beyond it stay
 * correct through the overflow list (global atomics).  Small bounds (1 in 3D; 1..4 in 2D) select the gather-form
 * adjoint (no atomics, bit-reproducible); larger ones the source-tiled window scatter (float atomics between tiles; the
 * LDS-tiled fixed-point scatter remains for reflection padding, C = 3 image warps and ADVCHAIN_WINDOW3D_MIN_HALO);
 * 0 = default scatter tiles (halo 2 in 3D) / window scatter (2D).
 * halo < 0: |halo| is EXACT -- the caller guarantees no sample moves |halo| voxels or more on any axis (measured with
 * advchain_max_displacement / disp_out): the gather form then skips the overflow list and is a single launch; samples
 * violating the guarantee would be dropped.  Exact bounds beyond the gather form (3D: 2..4 voxels; 2D: 4, 8, 16 px, squarings also 32 px; both
 * entries) select the owner-computes scatters of scatter_march.hip: LDS 32-bit fixed-point accumulators scaled by the
 * max|grad_out| over the rows a workgroup visits, plain stores, no zero fill, bit-reproducible, relative error of the
 * accumulation <= 2^-23 / 2^-22 / 2^-21 (bounds of 2 / 3 / 4; 2^-18 for 5..8) of that local maximum per deposit; a NaN / inf in
 * grad_out turns the outputs of the workgroups that visit its row into NaN (it is not dropped).  (Workspace word [3]: the
 * gather form leaves max|result| there, every scatter the mark -1; nothing reads it since the tiled scatter's scale became
 * local.) */
int advchain_compose_self_bwd(const float* grad_out, const float* phi, float* grad_phi, int32_t* workspace, int chain,
                              int halo, int64_t N, int ndim, const int64_t* dims, void* stream);
/* replaces: the loops of vectorFieldExponentiation{2,3}D (adv_morph.py:132-135,165-168) and their autograd, n squarings
 * in one call -- exactly the launches of n calls of advchain_compose_self_fwd / _bwd (same kernels, same results).
 * fwd: phi_1..phi_{n-1} -> fields[(n-1)][N][ndim][dims], the sampling positions (final_mode 1 of the last squaring)
 *      -> pos; disp_rows (may be NULL): (n+1) x ADVCHAIN_DISP_SLOTS zero-initialised floats, row m receives the
 *      displacement of phi_m (m >= 1; row 0 belongs to whoever made phi0), row n that of pos; hints (may be NULL): n
 *      displacement estimates in voxels (0 = unknown) for phi_0..phi_{n-1} (bits 0..7: as for advchain_grid_sample_fwd;
 *      bits 8..: the same estimate in 1/1024 voxel, 0 = unknown -- read by the 2D fusing rule).
 *      fuse_flag (may be NULL; TWO 32-bit words, ZERO before the call: a float flag and the arrival counter of the repeat
 *      launch's grid barrier): 2D only -- allows the leading squarings whose hinted input
 *      displacement is below one pixel, and the squarings behind them while the row halos of all fused levels (a level whose
 *      input moves less than h pixels needs h rows) sum to at most 5 (at most 5 levels, rows of 64k <= 512 pixels), to run as
 *      ONE launch over whole-row LDS windows (same arithmetic, bit-identical fields).  The kernel checks the premise on every window, level by level; a
 *      window that has to stop early records how many levels it could not do (*fuse_flag = the largest such count), and ONE
 *      repeat launch enqueued behind it (a persistent grid that returns at once while the flag is down) runs exactly those
 *      levels the ordinary way -- results never depend on the hints.  The caller may read the flag back (> 0: the hints were too optimistic) and must zero it
 *      before the next call.
 * bwd: grad_pos -> grad_phi0 through the n adjoint steps; halos[i] is the bound for the i-th step in BACKWARD order
 *      (squaring n-1 first); scratch: one field-sized buffer; workspace as for advchain_compose_self_bwd.             */
/* Query (host only, nothing is enqueued): how many leading squarings advchain_expo_chain_fwd would run as ONE fused launch for
 * this shape and these hints (0: none -- 3D, no hints, fewer than 256 windows, rows that are not a multiple of 64 pixels ...;
 * the pointer-alignment condition of the launch is not part of the answer).  Lets a caller / a test state which formulation
 * a chain takes; the reference has no counterpart (adv_morph.py:132-135 is one loop).                                  */
int advchain_expo_chain_fused_levels(int64_t N, int ndim, const int64_t* dims, int n, const int32_t* hints);
int advchain_expo_chain_fwd(const float* phi0, float* fields, float* pos, int64_t N, int ndim, const int64_t* dims, int n,
                            float* disp_rows, const int32_t* hints, float* fuse_flag, void* stream);
int advchain_expo_chain_bwd(const float* grad_pos, const float* phi0, const float* fields, float* grad_phi0, float* scratch,
                            int32_t* workspace, const int32_t* halos, int64_t N, int ndim, const int64_t* dims, int n,
                            void* stream);
/* Composite entries (round 5): ONE call enqueues a whole DemonsCompose direction for the paired field [v; -v] of a solver step
 * -- replaces: AdvMorph.DemonsCompose (adv_morph.py:454-491: Gaussian of the low-resolution velocity, F.interpolate, the
 * exponentiation of :116-146, composition with the identity grid, the final Gaussian) as the reference's forward() / backward()
 * call it (adv_morph.py:299-303,322-324), and its autograd.  2D, the 9-tap window, low-resolution planes of at most 4096
 * values.  The launches are exactly those of advchain_gauss_small_pair, advchain_tp_interp_fwd, advchain_expo_chain_fwd,
 * advchain_gauss_xy, advchain_slot_rows_max (forward) and advchain_gauss_xy, advchain_expo_chain_bwd,
 * advchain_band_reduce_rows_dense / _axis, advchain_gauss_small_pair (backward) in that order: same results, one trip out of
 * the host language per direction instead of five or six.  Every buffer is the caller's: s1 (2N, d, g...), phi0 / pos / q /
 * gpos / g / scratch (2N, d, S...), fields (n-1, 2N, d, S...), disp ((n+2) x ADVCHAIN_DISP_SLOTS, zero) + rows_max (n+2) or both
 * NULL, t1 (2N, d, S0, g1), gs1 (2N, d, g...), gvel (N, d, g...); tables as for advchain_tp_interp_fwd (3 axes, trivial leading
 * one), wd / wlo / WB: the densified innermost bands of advchain_band_reduce_rows_dense.  Returns ADVCHAIN_ERR_UNSUPPORTED (-2)
 * with NOTHING enqueued when a launch would not take the shape: issue the separate calls then.                              */
int advchain_demons_compose_pair_fwd(const float* vel, float* s1, float* phi0, float* fields, float* pos, float* q,
                                     float* disp, float* rows_max, const int32_t* itab, const float* ftab,
                                     const int64_t* S3, const int64_t* g3, const int64_t* B3, int64_t N, int ndim, int n,
                                     const int32_t* hints, const float* weights9_host, float scale, float inv, int fuse,
                                     void* stream);
int advchain_demons_compose_pair_bwd(const float* gq_lo, const float* gq_hi, const float* pos, const float* phi0,
                                     const float* fields, float* gpos, float* g, float* scratch, int32_t* ws, float* t1,
                                     float* gs1, float* gvel, const int32_t* halos, const int32_t* itab, const float* ftab,
                                     const float* wd, const int32_t* wlo, int64_t WB, const int64_t* S3, const int64_t* g3,
                                     const int64_t* B3, int64_t N, int ndim, int n, const float* weights9_host, float scale,
                                     float inv, void* stream);
/* max over samples and axes of |sampling position - own voxel| of the field phi, in voxels: the displacement
 * bound `halo` above wants.  out: one float, zero-initialised by the caller (atomic max).            */
int advchain_max_displacement(const float* phi, float* out, int64_t N, int ndim, const int64_t* dims, void* stream);
/* out[r] = max over the `cols` accumulator slots of row r (replaces torch.max(dim=1) on the (squarings + 1) x
 * ADVCHAIN_DISP_SLOTS tensor the squaring chain fills: 3 us instead of a 13-us two-pass reduction, 12 times per call);
 * NaN propagates.                                                                                        */
/* reset != 0: the slots are zeroed after they are read, so that one persistent accumulator serves every chain (no
 * zero-fill launch per chain). */
int advchain_slot_rows_max(float* slots, float* out, int64_t rows, int64_t cols, int reset, void* stream);
/* Premise check of a replayed launch plan (hipGraph replay of a solver call, INTEGRATION.md "Graph replay"): the reference
 * has no counterpart -- its ATen call sites (adv_morph.py:116-202, 546-557) do not choose between formulations.  The backward
 * kernels above are chosen from displacement bounds; a replayed plan froze that choice, and this entry compares what the
 * replay measures (`values`: advchain_slot_rows_max / advchain_max_displacement output, or the 3D step-rule norm of
 * adv_morph.py:159-162) with the frozen interval: flag[0] |= 1 when some values[i] is outside [lo[i], hi[i]) or NaN.  */
int advchain_bounds_check(const float* values, const float* lo, const float* hi, int64_t n, int32_t* flag, void* stream);

/* ---- affine warp -----------------------------------------------------------------------
 * replaces: F.affine_grid(theta, size, align_corners=True) + F.grid_sample(...),
 *           adv_affine.py:297-313.  theta (N, ndim, ndim+1); the grid is never materialised.    */
int advchain_affine_warp_fwd(const float* in, const float* theta, float* out, int64_t N, int64_t C, int ndim,
                             const int64_t* dims, int interp, int padding, void* stream);
/* advchain_affine_warp_fwd for two tensors under ONE theta: out = warp(in), ride_out = warp(ride_in) (one channel); see
 * advchain_grid_sample_fwd_ride (adv_affine.py:297-313 called for the data and for the validity mask,
 * adv_compose_solver.py:262-268).  Linear / zeros / rows of 16 bytes: one launch in 2D and 3D; otherwise two.         */
int advchain_affine_warp_fwd_ride(const float* in, const float* theta, float* out, const float* ride_in, float* ride_out,
                                  int64_t N, int64_t C, int ndim, const int64_t* dims, int interp, int padding, int flags,
                                  void* stream);
int64_t advchain_affine_warp_bwd_workspace(int64_t N, int ndim, const int64_t* dims); /* floats */
/* grad_in (N,C,dims) and grad_theta (N, ndim, ndim+1) are overwritten; either may be NULL.  grad_theta uses a
 * deterministic two-stage reduction.  grad_in: for linear interpolation with zeros padding and C <= 4 it is an
 * owner-computes scatter into LDS fixed-point accumulators (no global atomics, deterministic; scaled by the largest
 * |grad_out| around the tile -- taken from the theta-gradient walk, which runs first when both are asked for), for
 * C <= 8 a gather over the affine lattice; otherwise it is zero-filled here and scattered with atomics.
 * `workspace` (advchain_affine_warp_bwd_workspace floats) is always required.                                   */
int advchain_affine_warp_bwd(const float* grad_out, const float* in, const float* theta, float* grad_in,
                             float* grad_theta, float* workspace, int64_t N, int64_t C, int ndim,
                             const int64_t* dims, int interp, int padding, void* stream);
/* Deterministic twin of the scatter the call above falls back to (C > 8, nearest, or non-zeros padding): every sample's
 * grad_in deposits go through the int64 image of advchain_grid_sample_bwd_det (`det_ws`:
 * int32[advchain_det_warp_workspace(N, C, ndim, dims)], required when grad_in is asked for); grad_theta keeps the block
 * partials and the fixed-order second stage of that scatter and comes out bit for bit as from it.  Any C >= 1; for the
 * shapes the call above serves without atomics (C <= 8, linear, zeros) it is correct but slower and its grad_theta is
 * the scatter kernel's, not the box kernel's.  `workspace` as above.  Independent of the process-wide switch.          */
int advchain_affine_warp_bwd_det(const float* grad_out, const float* in, const float* theta, float* grad_in,
                                 float* grad_theta, float* workspace, int32_t* det_ws, int64_t N, int64_t C, int ndim,
                                 const int64_t* dims, int interp, int padding, void* stream);

/* ---- bicubic sampling (2D) ----------------------------------------------------------------
 * replaces: F.grid_sample(data, grid, mode='bicubic', padding_mode, align_corners=True), reached through the
 *           forward_interp / backward_interp config keys (adv_morph.py:255-258,546-557; adv_affine.py:297-313; ATen has
 *           no 5-D bicubic: 2D only).  Cubic convolution, A = -0.75, every tap's coordinate padded on its own.
 * in (N,C,H,W), grid (N,2,OH,OW) planar, out (N,C,OH,OW).  bwd: grad_in is zero-filled here and accumulated with
 * atomics, grad_grid overwritten; either may be NULL.                                                              */
int advchain_grid_sample_bicubic2d_fwd(const float* in, const float* grid, float* out, int64_t N, int64_t C,
                                       const int64_t* in_dims, const int64_t* out_dims, int padding, void* stream);
int advchain_grid_sample_bicubic2d_bwd(const float* grad_out, const float* in, const float* grid, float* grad_in,
                                       float* grad_grid, int64_t N, int64_t C, const int64_t* in_dims,
                                       const int64_t* out_dims, int padding, void* stream);
/* Deterministic twin of advchain_grid_sample_bicubic2d_bwd (all three paddings, in_dims != out_dims, any C >= 1).
 * replaces: the same grid_sampler_2d_backward (bicubic), as torch.use_deterministic_algorithms() would want it.
 * grad_in goes through an int64 fixed-point image with the passes of advchain_grid_sample_bwd_det (clear, max |grad_out| per
 * batch entry, 64-bit integer deposits, convert): equal bits run to run; a NaN / inf in an entry's grad_out turns that entry's
 * grad_in into NaN and leaves the other entries alone.  Width of the fixed point: a deposit is grad_out * cx * cy, and for
 * A = -0.75 the cubic weights satisfy |cx|, |cy| <= 1 (cubic1 falls from 1 to 0 on [0, 1]; cubic2 = A (x - 1)(x - 2)^2 has its
 * extreme -1/9 at x = 4/3), so a deposit is at most max|grad_out| = 2^bits units; border / reflection padding can fold all 16
 * taps of an output pixel onto one cell, so a cell receives at most 16 OH OW deposits, and
 *     bits = min(40, 62 - ceil(log2(16 OH OW)))
 * keeps every sum below 2^62 (quantum max|grad_out| / 2^bits per deposit).  det_ws:
 * int32[advchain_bicubic2d_det_workspace(N, C, in_dims)] = 2 N C H W for the image + N maxima padded to a multiple of 4,
 * 8-byte aligned (an odd C H W is fine: the image is converted with 8-byte loads); host-only size query, independent of the
 * switch; required when grad_in is asked for.  grad_in is overwritten (no pre-zeroing).  grad_grid is bit for bit what
 * advchain_grid_sample_bicubic2d_bwd writes: that very kernel is launched for it with grad_in = NULL, and the deposits are
 * a launch of their own.  Works whatever advchain_get_deterministic() says.                                            */
int64_t advchain_bicubic2d_det_workspace(int64_t N, int64_t C, const int64_t* in_dims); /* int32 elements */
int advchain_grid_sample_bicubic2d_bwd_det(const float* grad_out, const float* in, const float* grid, float* grad_in,
                                           float* grad_grid, int32_t* det_ws, int64_t N, int64_t C, const int64_t* in_dims,
                                           const int64_t* out_dims, int padding, void* stream);
/* replaces: F.affine_grid(theta, size, align_corners=True) for the bicubic affine warp (adv_affine.py:297-305): theta
 *           (N,2,3) -> planar grid (N,2,H,W), and its adjoint grad_grid -> grad_theta (deterministic two-stage sum;
 *           workspace: advchain_affine_grid2d_bwd_workspace floats).                                                */
int advchain_affine_grid2d_fwd(const float* theta, float* grid, int64_t N, const int64_t* dims, void* stream);
int64_t advchain_affine_grid2d_bwd_workspace(int64_t N, const int64_t* dims);
int advchain_affine_grid2d_bwd(const float* grad_grid, float* grad_theta, float* workspace, int64_t N, const int64_t* dims,
                               void* stream);

/* ---- affine parameters -> matrices -----------------------------------------------------
 * replaces: AdvAffine.gen_batch_affine_matrix adv_affine.py:210-273 (Hardtanh, Euler z-y'-x''
 *           rotation, scale, translation) and get_inverse_matrix adv_affine.py:316-324.
 * param (N, 5|9); cfg = 2D {rot, scale_x, scale_y, shift_x, shift_y}
 *                       3D {rot_x,rot_y,rot_z, scale_x,scale_y,scale_z, shift_x,shift_y,shift_z};
 * theta, theta_inv (N, ndim, ndim+1).                                                         */
int advchain_affine_theta_fwd(const float* param, const float* cfg_host, float param_scale, float* theta,
                              float* theta_inv, int64_t N, int ndim, void* stream);
int advchain_affine_theta_bwd(const float* param, const float* cfg_host, float param_scale, const float* grad_theta,
                              const float* grad_theta_inv, float* grad_param, int64_t N, int ndim, void* stream);

/* ---- banded tensor-product interpolation -----------------------------------------------
 * Band tables (see advchain_amd/bands.py) describe, per axis a of the padded 3-axis view
 * (2D passes a trivial leading axis), a linear map from g_a coefficients to S_a samples with at
 * most B_a (<= 8) contiguous non-zeros per sample:
 *   itab = for a in 0..2: start[S_a] | lo[g_a] | hi[g_a]      (int32)
 *   ftab = for a in 0..2: w[S_a * B_a]                        (fp32)
 * replaces: F.interpolate(duv, size=full, 'bilinear'|'trilinear', align_corners=False)
 *           adv_morph.py:464, fused with 'basegrid += duv/2^n' (adv_morph.py:111,129-130) when
 *           add_identity != 0, and with torch.norm(duv_interval) (adv_morph.py:160) when
 *           sumsq != NULL (64 partial accumulators: sum(sumsq[0..63]) += sum(interp^2); caller zeroes them).
 * coef (planes, g0,g1,g2) -> out (planes, S0,S1,S2) = identity? + scale * interp.
 * disp_out (may be NULL): ADVCHAIN_DISP_SLOTS floats, max-accumulates |scale * interp| in voxels, i.e. the displacement
 * of the field written when add_identity != 0 (see advchain_compose_self_fwd).                          */
int advchain_tp_interp_fwd(const float* coef, float* out, const int32_t* itab, const float* ftab, const int64_t* S,
                           const int64_t* g, const int64_t* B, int64_t planes, int64_t C, int ndim, int add_identity,
                           float scale, float* sumsq, float* disp_out, void* stream);
/* The sum of squares of the call above (out = NULL, sumsq) in a FIXED ORDER (deterministic mode).
 * replaces: torch.norm(duv_interval) ** 2 of vectorFieldExponentiation3D (adv_morph.py:159-162), a deterministic function of
 *           its input in the reference.  The kernel advchain_tp_interp_fwd would pick writes one partial per workgroup into
 *           `partials` (at least advchain_tp_interp_sumsq_partials(S, planes) = ceil(S[1] / 32) * S[0] * planes floats: the most
 *           workgroups such a launch has; host-only query, -1 for bad sizes; no clearing needed) and one workgroup adds them
 *           in a fixed order into out[0].  The field is not materialised.  Works whatever the switch says.            */
int64_t advchain_tp_interp_sumsq_partials(const int64_t* S, int64_t planes); /* floats */
int advchain_tp_interp_sumsq_ordered(const float* coef, const int32_t* itab, const float* ftab, const int64_t* S, const int64_t* g,
                                     const int64_t* B, int64_t planes, int64_t C, float* partials, float* out, void* stream);
/* advchain_gauss_small_pair (forward) + advchain_tp_interp_fwd in ONE launch (round 6) for the paired 2D field [v; -v].
 * replaces: the first two steps of AdvMorph.DemonsCompose -- the Gaussian of the low-resolution velocity (adv_morph.py:377-452,
 *           called at :460-462) and F.interpolate to full size (adv_morph.py:464) -- for forward() / backward() of one solver
 *           step (adv_morph.py:299-303,322-324).  vel: (P planes of g1 x g2 values); s1 (may be NULL): (2P planes) receives the
 *           smoothed batch [G(gscale v); G(-gscale v)]; out: (2P planes of S1 x S2) = (add_identity ? identity : 0) + scale * up(s1);
 *           disp_out as for advchain_tp_interp_fwd.  Same arithmetic as the two calls, bit for bit.  2D tables (trivial leading
 *           axis), low-resolution planes of at most 1024 values, the 9-tap window; ADVCHAIN_ERR_UNSUPPORTED (-2) with nothing
 *           enqueued otherwise.                                                                                              */
int advchain_tp_interp_fwd_smoothed_pair(const float* vel, float* s1, float* out, const int32_t* itab, const float* ftab,
                                         const int64_t* S, const int64_t* g, const int64_t* B, int64_t P, int64_t C,
                                         int add_identity, float scale, float* disp_out, const float* weights9, float gscale,
                                         void* stream);
/* The same with the i1 rows a workgroup takes as an argument: rows_per_wg in {4, 8, 16, 32}, or 0 for the library's choice
 * (32; the entry above passes 0).  Every output bit is the same whatever the value -- for the row sweeps of the tools.       */
int advchain_tp_interp_fwd_smoothed_pair_rows(const float* vel, float* s1, float* out, const int32_t* itab, const float* ftab,
                                              const int64_t* S, const int64_t* g, const int64_t* B, int64_t P, int64_t C,
                                              int add_identity, float scale, float* disp_out, const float* weights9, float gscale,
                                              int rows_per_wg, void* stream);
/* adjoint along one axis: in (outer, S_axis, inner) -> out (outer, g_axis, inner),
 * out = W_axis^T ((in - in2) * scale); in2 may be NULL.
 * replaces: upsample_{bi,tri}linear backward / conv_transpose backward w.r.t. its input.        */
int advchain_band_reduce_axis(const float* in, const float* in2, float* out, const int32_t* itab, const float* ftab,
                              const int64_t* S, const int64_t* g, const int64_t* B, int axis, int64_t outer,
                              int64_t inner, float scale, void* stream);
/* The innermost-axis pass of the same adjoint (inner == 1: the full-resolution pass, which reads the whole gradient once) with
 * the bands densified by the caller once per table: wd[g][WB] = weight of input lo[k] + j for coefficient k (zero beyond its
 * band), lo[g].  in: (rows, S) [minus in2] -> out: (rows, g) * scale.  Returns ADVCHAIN_ERR_UNSUPPORTED (-2) for shapes it
 * does not take (S % 4 != 0, S > 1024, g > 64, g * WB > 4096, unaligned inputs): use advchain_band_reduce_axis then.
 * Same sums in the same order as that entry. */
int advchain_band_reduce_rows_dense(const float* in, const float* in2, float* out, const float* wd, const int32_t* lo,
                                    int64_t rows, int64_t S, int64_t g, int64_t WB, float scale, void* stream);
/* How the row-blended kernels (advchain_tp_interp_fwd, _smoothed_pair, the bias field entries below) fetch their band tables
 * where a thread produces four columns: 16-byte requests for innermost bands of 2 or 4 (the default), or dword loads for
 * every band (on = 0).  Process-wide, host-only; every output bit is the same either way -- for tests and tools that compare
 * the two forms in one process.                                                                                              */
void advchain_set_tp_wide_loads(int on);
int advchain_get_tp_wide_loads(void);
/* The band width whose 16-byte form a table with innermost band B2 takes at the moment (2 or 4), 0 for the dword loads. */
int advchain_tp_wide_band(int64_t B2);

/* ---- bias field ------------------------------------------------------------------------
 * replaces: AdvBias.compute_smoothed_bias + clip_bias + multiply, adv_bias.py:279-356,186:
 *           conv_transpose{2,3}d(cp, bspline) -> crop -> Upsample(linear, align_corners=False)
 *           -> exp (log space) or 1+x -> 1+clamp(b-1,-eps,eps) -> data*b, evaluated in closed
 *           form from the control points (band tables = upsample o B-spline, per axis).
 * cp (N,1,g...), data/out (N,C,S...), field (N,1,S...) = clipped bias.  data may be NULL.        */
int advchain_bias_field_fwd(const float* cp, const float* data, float* out, float* field, const int32_t* itab,
                            const float* ftab, const int64_t* S, const int64_t* g, const int64_t* B, int64_t N,
                            int64_t C, float eps, int use_log, float cp_scale, void* stream);
/* grad_L (N,1,S...) = dLoss/d(log-field) at full resolution (reduce to control points with
 * advchain_band_reduce_axis); grad_data (N,C,S...) = grad_out * field.  Either may be NULL.     */
int advchain_bias_field_bwd(const float* cp, const float* data, const float* grad_out, float* grad_L, float* grad_data,
                            const int32_t* itab, const float* ftab, const int64_t* S, const int64_t* g,
                            const int64_t* B, int64_t N, int64_t C, float eps, int use_log, float cp_scale,
                            void* stream);
/* The two entries above with the i1 rows a workgroup takes as an argument: rows_per_wg in {4, 8, 16, 32}, or 0 for the
 * library's rule, advchain_bias_rows_per_wg(S, N) (host-only; S: 3 entries, 2D a leading 1; -1 for bad arguments) -- the
 * largest of the four values that still gives the launch 512 workgroups, else 4.  The entries above pass 0.  Every output bit
 * is the same whatever the value.                                                                                            */
int advchain_bias_rows_per_wg(const int64_t* S, int64_t N);
int advchain_bias_field_fwd_rows(const float* cp, const float* data, float* out, float* field, const int32_t* itab,
                                 const float* ftab, const int64_t* S, const int64_t* g, const int64_t* B, int64_t N,
                                 int64_t C, float eps, int use_log, float cp_scale, int rows_per_wg, void* stream);
int advchain_bias_field_bwd_rows(const float* cp, const float* data, const float* grad_out, float* grad_L, float* grad_data,
                                 const int32_t* itab, const float* ftab, const int64_t* S, const int64_t* g,
                                 const int64_t* B, int64_t N, int64_t C, float eps, int use_log, float cp_scale,
                                 int rows_per_wg, void* stream);
/* advchain_bias_field_bwd and the innermost pass of the adjoint over grad_L (advchain_band_reduce_rows_dense, scale 1) in one
 * launch: grad_L is never written; t1 (N, 1, S0, S1, g2) is what that pass would have produced from it, bit for bit (the
 * remaining axes: advchain_band_reduce_axis).  wd / lo / WB: the densified innermost bands, as for
 * advchain_band_reduce_rows_dense.  grad_data may be NULL.  Returns ADVCHAIN_ERR_UNSUPPORTED (-2), nothing enqueued, when
 * t1 is NULL, for the shapes advchain_band_reduce_rows_dense refuses (S2 % 4 != 0, S2 > 1024, g2 > 64, g2 * WB > 4096, data /
 * grad_out / grad_data not 16-byte aligned), or when the dense table and a slab of 4 rows of S2 + 1 floats exceed 48 KiB of
 * LDS (rows_per_wg is halved until table and slab fit): issue the two calls then.                                            */
int advchain_bias_field_bwd_reduced(const float* cp, const float* data, const float* grad_out, float* t1, float* grad_data,
                                    const int32_t* itab, const float* ftab, const int64_t* S, const int64_t* g,
                                    const int64_t* B, int64_t N, int64_t C, float eps, int use_log, float cp_scale,
                                    const float* wd, const int32_t* lo, int64_t WB, int rows_per_wg, void* stream);

/* ---- separable Gaussian ----------------------------------------------------------------
 * replaces: depthwise nn.Conv{2,3}d with the normalised 9^d Gaussian (sigma=1), zero padding,
 *           adv_morph.py:377-452; one axis per call (self-adjoint: same entry for backward).
 * pre : 0 none | 1 x*scale | 2 F.grid_sample(base_grid, x, 'border') - base_grid  (adv_morph.py:473-487)
 * post: 0 none | 1 + base_grid (adv_morph.py:489)   | 2 * d(pre 2)/dx at aux      (backward of pre 2)
 * in/out/aux (planes, dims); plane p carries grid channel p % C.  host pointer weights9[9].     */
int advchain_gauss_axis(const float* in, float* out, const float* aux, int64_t planes, int64_t C, int ndim,
                        const int64_t* dims, int axis, const float* weights9_host, int pre, int post, float scale,
                        void* stream);

/* The same convolution with ANY odd window (host pointer weights[ntaps], 1 <= ntaps <= 129): the reference sizes its window
 * as 2 * int(4 sigma + 0.5) + 1 taps (adv_morph.py:393-398), 9 only for 0.875 <= sigma < 1.125; out = G_axis * (scale * in),
 * zero padding, no prologue / epilogue.  Plain per-voxel form (the reference never leaves sigma = 1).                       */
int advchain_gauss_axis_generic(const float* in, float* out, int64_t planes, int ndim, const int64_t* dims, int axis,
                                const float* weights_host, int ntaps, float scale, void* stream);

/* x and y passes of the Gaussian above in ONE launch (LDS tile of whole rows): one read and one write of the tensor
 * instead of two each; the same sums in the same tap order as the two per-axis calls (results agree to a few ulp).  post != 0 only when y is the last axis (ndim == 2).
 * Returns -2 (unsupported, no error text) for shapes it does not take (rows not a multiple of 4 or longer than 512, unaligned
 * tensors): run advchain_gauss_axis for axes 2 and 1 then.
 * in_hi (may be NULL): the input planes [planes_lo, planes) come from this second tensor (the gradient of a paired field
 * arrives as two halves), in: planes [0, planes_lo).                                                                    */
int advchain_gauss_xy(const float* in, float* out, const float* aux, int64_t planes, int64_t C, int ndim, const int64_t* dims,
                      const float* weights9, int pre, int post, float scale, void* stream, const float* in_hi,
                      int64_t planes_lo);
/* advchain_gauss_xy has two kernels with the same results bit for bit.  The staged form (x pass LDS -> LDS) takes every shape
 * above.  The lane form takes rows that never straddle a wave (rows of 8, 16, 32, 64, 128 or 256 voxels): the x taps come from
 * the neighbouring lanes, half the LDS, one barrier; advchain_gauss_xy runs it where it was measured to win, rows of 256 voxels
 * (32 rows and 512 threads a workgroup), and the staged form everywhere else.
 * advchain_gauss_xy_staged: always the staged form (the reference of the tests).
 * advchain_gauss_xy_lanes: the lane form with ty rows and nt threads a workgroup, (ty, nt) one of (16,256), (16,512), (32,256),
 * (32,512), (64,1024); -2 for a shape the lane form does not take.
 * advchain_gauss_xy_plan (host-only): what advchain_gauss_xy does with a launch, pointer alignment aside -- *form 0: not taken,
 * 1: staged, 2: lanes; *ty rows and *nt threads a workgroup.  Returns 0, -1 for bad arguments.                             */
int advchain_gauss_xy_staged(const float* in, float* out, const float* aux, int64_t planes, int64_t C, int ndim,
                             const int64_t* dims, const float* weights9, int pre, int post, float scale, void* stream,
                             const float* in_hi, int64_t planes_lo);
int advchain_gauss_xy_lanes(const float* in, float* out, const float* aux, int64_t planes, int64_t C, int ndim,
                            const int64_t* dims, const float* weights9, int pre, int post, float scale, void* stream,
                            const float* in_hi, int64_t planes_lo, int ty, int nt);
int advchain_gauss_xy_plan(int ndim, const int64_t* dims, int64_t planes, int* form, int* ty, int* nt);
/* all axes of the same Gaussian in ONE launch for small planes (<= 4096 voxels: the low-resolution velocity grids,
 * adv_morph.py:462-463); pre = 0 | 1 (x * scale), no epilogue; same arithmetic as the per-axis calls.              */
int advchain_gauss_small(const float* in, float* out, int64_t planes, int ndim, const int64_t* dims,
                         const float* weights9_host, int pre, float scale, void* stream);

/* The same for the batch [v; -v] of a paired field (the deformation and its approximate inverse of one solver step,
 * adv_morph.py:285-331) without materialising the negated copy: adjoint == 0: in (planes), out (2 planes): out[p] =
 * G(scale in[p]), out[planes + p] = G(-scale in[p]) (bit-identical to smoothing a negated copy); adjoint != 0: in
 * (2 planes), out (planes): out[p] = G(scale in[p]) - G(scale in[planes + p]).                                       */
int advchain_gauss_small_pair(const float* in, float* out, int64_t planes, int ndim, const int64_t* dims,
                              const float* weights9_host, float scale, int adjoint, void* stream);

/* ---- streaming / per-sample normalisation ----------------------------------------------
 * replaces: data + eps*param adv_noise.py:81-84 (x may be NULL: out = a*y).                     */
int advchain_axpy(const float* x, const float* y, float* out, float a, int64_t n, void* stream);
/* replaces: param + step * grad.sign() (adv_affine.py:186-195); base may be NULL (power iteration: sign only).   */
/* gate (may be NULL): a device scalar (the loss of the step); when it is NaN / inf the update is void and out = old --
 * the NaN guard of the ascent loop (adv_compose_solver.py:343-347) evaluated on the device, so that the host does not have
 * to read the loss back in the middle of a step.                                                                      */
int advchain_sign_axpy(const float* base, const float* x, float* out, float a, int64_t n, const float* gate, const float* old,
                       void* stream);
/* replaces: fb[fb != 0] = 1 of the validity mask (adv_compose_solver.py:266-268,323-325): out = (x != 0) ? 1 : 0.  */
int advchain_nonzero_mask(const float* x, float* out, int64_t n, void* stream);
int64_t advchain_norm_workspace(int64_t N, int64_t M); /* floats */
/* replaces: unit_normalize (adv_transformation_base.py:151-155) fused with the ascent update
 *           param + step*g/(||g||+1e-20) (adv_noise.py:56-63, adv_bias.py:144-147,
 *           adv_morph.py:511-513).  base may be NULL (pure normalisation).  x (N, M).           */
int advchain_norm_axpy(const float* base, const float* x, float* out, float* workspace, float step, int64_t N,
                       int64_t M, void* stream);
/* the same with the NaN gate of advchain_sign_axpy */
int advchain_norm_axpy_gated(const float* base, const float* x, float* out, float* workspace, float step, int64_t N,
                             int64_t M, const float* gate, const float* old, void* stream);
/* The parameter updates of ONE ascent step in ONE launch (round 6).
 * replaces: the per-transform optimize_parameters() calls at the end of a step (adv_compose_solver.py:349-364 ->
 *           adv_noise.py:51-64, adv_bias.py:139-148, adv_morph.py:501-516: param + step * unit_normalize(grad);
 *           adv_affine.py:182-198: param + step * sign(grad)) and the NaN guard of adv_compose_solver.py:343-347 -- what
 *           advchain_norm_axpy_gated / advchain_sign_axpy do one transform at a time.  descs: n <= 8 HOST descriptors;
 *           kind 0: out[r] = (base ? base[r] : 0) + step * x[r] / (||x[r]||_2 + 1e-20) per row r of M values; kind 1: the sign
 *           step.  gate (may be NULL): a device scalar; when it is NaN / inf every `out` receives `old` (required then).
 *           One workgroup per row: same formula as the separate entries, square sums in a different order (rounding).   */
typedef struct advchain_update_desc {
  const float* base;
  const float* x;
  float* out;
  const float* old;
  int64_t N;
  int64_t M;
  int32_t kind;
  float step;
} advchain_update_desc;
int advchain_update_multi(const advchain_update_desc* descs, int n, const float* gate, void* stream);

/* ---- consistency loss ------------------------------------------------------------------
 * replaces: calc_segmentation_consistency / contour_loss / kl_divergence, advchain/common/loss.py:8-87,102-220,223-249
 *           ('mse', 'contour' and 'kl' terms: softmax over K, mask, 3^d edge stencils, Q13/Q14).
 * pred/ref (N,K,dims) logits (ref already a probability map when ref_is_prob), mask
 * (N, mask_channels in {1,K}, dims) or NULL.  Outputs: P = softmax(pred), D = P - T (N,K,dims);
 * R (N, 2(K-1), dims) = 2 m^2 (A*D), 2 m^2 (B*D) per class 1..K-1 (NULL when no backward is
 * needed); sums is 4 x 64 partial accumulators (row r, slot s at sums[64 r + s]; per-workgroup partials are
 * spread over the slots because same-address atomics serialise): row 0 += sum ((P m)-(T m))^2, row 1 +=
 * sum (A*D m)^2, row 2 += sum (B*D m)^2, row 3 (want_kl != 0 only) += sum_k m_k T'_k (log T'_k - log P_k) with
 * T' = T, or where(ref == 0, 1e-8, 1 - 1e-8) when ref_is_prob (loss.py:239-243) (caller zeroes `sums`, adds the slots up
 * and applies the GLOBAL normalisers -- required for batch sharding).  2D: A = Sobel-x, B = Sobel-y.
 * 3D: A = h(x)hp(x)h (the reference uses it for conv_x AND conv_y), B = h(x)h(x)hp.                */
int advchain_consistency_fwd(const float* pred, const float* ref, const float* mask, float* P, float* D, float* R,
                             float* sums, int64_t N, int64_t K, int ndim, const int64_t* dims, int mask_channels,
                             int ref_is_prob, int want_edges, int want_kl, void* stream);
/* replaces: the sums and the weighted total of calc_segmentation_consistency (loss.py:80-87): sums[r] = sum of the 64
 * slots of row r (4 floats), value[0] = sum_r coef4[r] * sums[r]; reset != 0 zeroes the slots for the next call.  */
int advchain_consistency_finish(float* slots, const float* coef4_host, float* sums, float* value, int reset, void* stream);
/* grad_pred (N,K,dims) = softmax'(P)[ gs (c_mse 2 m^2 D + c_a A^T R_A + c_b B^T R_B) ]
 *                        + gs c_kl (P_j sum_k m_k T'_k - m_j T'_j),   gs = *grad_scale (device scalar, NULL = 1);
 * the 'kl' term (c_kl != 0) rebuilds T' from P - D (kl_is_gt: the where() of the forward).        */
int advchain_consistency_bwd(const float* P, const float* D, const float* R, const float* mask,
                             const float* grad_scale, float* grad_pred, float c_mse, float c_a, float c_b, float c_kl,
                             int kl_is_gt, int64_t N, int64_t K, int ndim, const int64_t* dims, int mask_channels,
                             void* stream);
/* f2, fused (round 4): the same loss without its per-voxel intermediates.  fused_fwd: softmax(pred), softmax(ref) (or ref
 * itself), the masked squared error, the KL sum and the 3^d edge stencils in ONE marching kernel straight from the logits;
 * it writes only R (2(K-1) channels; may be NULL when no gradient is wanted) and adds to the same 4 x 64 slot sums as
 * advchain_consistency_fwd (finish with advchain_consistency_finish).  fused_bwd: grad_pred from pred, ref, R -- the softmax is
 * recomputed at the voxel instead of reading P and D back.  Same per-voxel arithmetic as the unfused entries (replaces the
 * same reference lines: common/loss.py:8-87,102-220,223-249).  Both return ADVCHAIN_ERR_UNSUPPORTED (-2) for what the 16-byte
 * marching form does not take -- rows of 4j <= 256 voxels, K = 2..4, a mask of at most one channel, 16-byte aligned
 * tensors: use the unfused entries then.  3D (round 5): with the edge terms wanted and rows of at most 128 voxels the march goes
 * along z with the y neighbours of a row exchanged through LDS (every logit is read ~1.4 x instead of 3.75 x); other 3D calls
 * return -2 as before. */
int advchain_consistency_fused_fwd(const float* pred, const float* ref, const float* mask, float* R, float* sums, int64_t N,
                                   int64_t K, int ndim, const int64_t* dims, int mask_channels, int ref_is_prob, int want_edges,
                                   int want_kl, void* stream);
int advchain_consistency_fused_bwd(const float* pred, const float* ref, const float* R, const float* mask,
                                   const float* grad_scale, float* grad_pred, float c_mse, float c_a, float c_b, float c_kl,
                                   int ref_is_prob, int64_t N, int64_t K, int ndim, const int64_t* dims, int mask_channels,
                                   void* stream);

/* wide (round 8): the same loss for a RUN-TIME class count, 1 <= K < 65536 -- nothing in these kernels is sized by K
 * (replaces the same reference lines: common/loss.py:8-87,102-220,223-249; same terms, masks, ref_is_prob and slot sums as
 * advchain_consistency_fwd, finish with advchain_consistency_finish).  wide_fwd: one streaming pass leaves the softmax
 * statistics of both operands in stats (N, 4, dims) floats = max_pred, 1 / sum_pred, max_ref, 1 / sum_ref (the ref planes are
 * unspecified when ref_is_prob) and adds the 'mse' and 'kl' sums; with want_edges and K > 1 a tiled kernel marching over the
 * classes adds the edge energies and writes R (N, 2(K-1), dims) as above (NULL when no backward is needed).  P and D are
 * never materialised.  wide_bwd: grad_pred (N,K,dims) from pred, ref, stats and R (NULL: no edge terms) by the formula of
 * advchain_consistency_bwd, gs = *grad_scale (device scalar, NULL = 1); no atomics on grad_pred, so it is bit-reproducible.
 * pred / ref / grad_pred fp32 contiguous, any alignment (16-byte aligned tensors with a voxel count divisible by 4 take
 * 16-byte loads; a lane owns the same 4 voxels either way, so no sum, and with it no value, depends on the alignment of a
 * tensor); N < 65536 (N == 0: ADVCHAIN_OK, no launch), fewer than 2^31 voxels, mask_channels 1 or K.  Capture-safe: kernel
 * launches on `stream` only.  Returns ADVCHAIN_OK or a negative code (advchain_last_error names the entry).
 * These entries (and advchain_consistency_wide_fwd_partials / wide_fwd_ord below) ARE the lp entries further down with both
 * storage flags 0 and no class weights -- the same kernels (loss_lp.hip), stats and R interchangeable with theirs -- under the
 * fp32 signatures. */
int advchain_consistency_wide_fwd(const float* pred, const float* ref, const float* mask, float* stats, float* R, float* sums,
                                  int64_t N, int64_t K, int ndim, const int64_t* dims, int mask_channels, int ref_is_prob,
                                  int want_edges, int want_kl, void* stream);
int advchain_consistency_wide_bwd(const float* pred, const float* ref, const float* stats, const float* R, const float* mask,
                                  const float* grad_scale, float* grad_pred, float c_mse, float c_a, float c_b, float c_kl,
                                  int ref_is_prob, int64_t N, int64_t K, int ndim, const int64_t* dims, int mask_channels,
                                  void* stream);

/* reference side (round 9): grad_ref (N,K,dims) = what autograd gives `reference` in the same expression (call site
 * common/loss.py:8-87,223-249: calc_segmentation_consistency / kl_divergence with a reference that requires grad -- mutual
 * consistency of two branches, a symmetric KL term, a teacher trained through the term, a soft is_gt target).  With
 *   g_k = gs (c_mse 2 m_k^2 (P_k - T_k) + [k >= 1] (c_a A^T R_A,k + c_b B^T R_B,k))      (the probability-space gradient of
 *                                                                                         advchain_consistency_bwd)
 *   h_k = -g_k + gs c_kl m_k (log T_k + 1 - log P_k)
 * ref_is_prob == 0: grad_ref_k = T_k (h_k - sum_j T_j h_j) (softmax Jacobian of the reference; log T_k - log P_k is taken from
 * the logits and the softmax statistics); ref_is_prob != 0: grad_ref_k = -g_k -- the reference's where() cuts the graph of
 * 'kl', c_kl is ignored and the reference's softmax is never evaluated (with 'kl' alone the gradient is zero: do not call).
 * Independent of the forward family: pred, ref, mask as given to the forward, R (N, 2(K-1), dims) as any forward entry wrote
 * it (NULL: no edge terms or K == 1), stats (N, 4, dims) as advchain_consistency_wide_fwd wrote it or NULL (the kernel then
 * takes the softmax statistics of its own output voxels in a sweep over the classes; it never touches the slot sums).
 * gs = *grad_scale (device scalar, NULL = 1).  K = 2..4 keep a thread's logits in registers and read every operand once;
 * other K (or all K after advchain_set_ref_grad_reg_max_k(0): PROCESS-WIDE, 0..4, default 4; for tests and A/B) march over
 * the classes twice with grad_ref as the only scratch.  No atomics: bit-reproducible in either form.  pred / ref / grad_ref
 * fp32 contiguous, any alignment; N < 65536 (N == 0: ADVCHAIN_OK, no launch), 1 <= K < 65536, fewer than 2^31 voxels,
 * mask_channels 1 or K.  Capture-safe: one kernel launch on `stream`.  Returns ADVCHAIN_OK or a negative code. */
int advchain_consistency_ref_bwd(const float* pred, const float* ref, const float* stats /*nullable*/,
                                 const float* R /*nullable*/, const float* mask, const float* grad_scale,
                                 float* grad_ref, float c_mse, float c_a, float c_b, float c_kl, int ref_is_prob,
                                 int64_t N, int64_t K, int ndim, const int64_t* dims, int mask_channels, void* stream);
void advchain_set_ref_grad_reg_max_k(int k);
int advchain_get_ref_grad_reg_max_k(void);

/* low-precision storage (round 10, loss_lp.hip): the same loss and both of its gradients for logits stored in bf16 (a model
 * under autocast), every K from 1 to 65535, 2D and 3D.  pred / ref are read as fp32 (flag 0) or as raw bf16 words (flag 1),
 * independently; bf16 -> fp32 is exact and all arithmetic is fp32 (the wide entries are these with both flags 0), so lp_fwd computes the
 * fp32 loss of the upcast operands.  mask, stats (N, 4, dims), R (N, 2(K-1), dims; NULL when no backward is needed) and the
 * slot sums are fp32 and have the layouts of advchain_consistency_wide_fwd (finish with advchain_consistency_finish); a
 * reference given as probabilities (ref_is_prob) is read in its own storage type as it is.  lp_bwd writes grad_pred in pred's
 * type, lp_ref_bwd writes grad_ref in ref's type (formulas of advchain_consistency_wide_bwd / advchain_consistency_ref_bwd;
 * stats must be what lp_fwd wrote, R NULL: no edge terms): computed in fp32 and rounded once, to nearest even, at the store.
 * The probability-space gradient between the two sweeps of a backward never passes through the output: the second sweep
 * recomputes it, so there is no scratch and no workspace.  No atomics on the gradients: bit-reproducible.  Tensors are
 * contiguous at any alignment (lp_fwd's streaming pass takes 16-byte fp32 / 8-byte bf16 accesses when the voxel count is
 * divisible by 4 and every pointer allows it; the value does not depend on which form ran).  N < 65536 (N == 0: ADVCHAIN_OK,
 * no launch), fewer than 2^31 voxels, mask_channels 1 or K, flags 0 or 1.  Capture-safe: kernel launches on `stream` only.
 * Returns ADVCHAIN_OK or a negative code (advchain_last_error names the entry). */
int advchain_consistency_lp_fwd(const void* pred, int pred_bf16, const void* ref, int ref_bf16, const float* mask, float* stats,
                                float* R /*nullable*/, float* sums, int64_t N, int64_t K, int ndim, const int64_t* dims,
                                int mask_channels, int ref_is_prob, int want_edges, int want_kl, void* stream);
int advchain_consistency_lp_bwd(const void* pred, int pred_bf16, const void* ref, int ref_bf16, const float* stats,
                                const float* R /*nullable*/, const float* mask, const float* grad_scale, void* grad_pred,
                                float c_mse, float c_a, float c_b, float c_kl, int ref_is_prob, int64_t N, int64_t K, int ndim,
                                const int64_t* dims, int mask_channels, void* stream);
int advchain_consistency_lp_ref_bwd(const void* pred, int pred_bf16, const void* ref, int ref_bf16, const float* stats,
                                    const float* R /*nullable*/, const float* mask, const float* grad_scale, void* grad_ref,
                                    float c_mse, float c_a, float c_b, float c_kl, int ref_is_prob, int64_t N, int64_t K,
                                    int ndim, const int64_t* dims, int mask_channels, void* stream);

/* class weights (round 11, loss_lp.hip): the lp entries with K finite, non-negative weights w_k in device memory (class_w, K
 * floats, not NULL; read by the kernels, so they must stay unchanged until the launches have run), used as given:
 *   S_mse = sum w_k (m_k D_k)^2,  S_kl = sum w_k m_k T'_k (log T'_k - log P_k),  edge energies of object class i times w_i
 * (w_0 does not enter 'contour'); every normaliser is the caller's, in the coefficients, as before.  w = 1 is the loss of the
 * lp entries.  The same kernels instantiated with a trailing weight argument: all four storage pairs (fp32-fp32 included), every
 * K, 2D and 3D, the layouts, limits, rounding and reproducibility of the lp entries; stats and R as cw_fwd wrote them (R is
 * saved unweighted, the backward entries scale the probability-space gradient of class k by w_k); finish with
 * advchain_consistency_finish.  The weights are constants: no gradient. */
int advchain_consistency_cw_fwd(const void* pred, int pred_bf16, const void* ref, int ref_bf16, const float* mask, float* stats,
                                float* R /*nullable*/, float* sums, int64_t N, int64_t K, int ndim, const int64_t* dims,
                                int mask_channels, int ref_is_prob, int want_edges, int want_kl, const float* class_w,
                                void* stream);
int advchain_consistency_cw_bwd(const void* pred, int pred_bf16, const void* ref, int ref_bf16, const float* stats,
                                const float* R /*nullable*/, const float* mask, const float* grad_scale, void* grad_pred,
                                float c_mse, float c_a, float c_b, float c_kl, int ref_is_prob, int64_t N, int64_t K, int ndim,
                                const int64_t* dims, int mask_channels, const float* class_w, void* stream);
int advchain_consistency_cw_ref_bwd(const void* pred, int pred_bf16, const void* ref, int ref_bf16, const float* stats,
                                    const float* R /*nullable*/, const float* mask, const float* grad_scale, void* grad_ref,
                                    float c_mse, float c_a, float c_b, float c_kl, int ref_is_prob, int64_t N, int64_t K,
                                    int ndim, const int64_t* dims, int mask_channels, const float* class_w, void* stream);

/* ---- the consistency loss with its sums in a fixed order (deterministic mode) -------------------------------------------
 * replaces: the same calc_segmentation_consistency / contour_loss / kl_divergence sums (common/loss.py:8-87,102-249), which are
 *           deterministic functions of their inputs in the reference's CPU path.
 * Each *_fwd_ord entry is its forward family's entry with `sums` (the 4 x 64 slots) replaced by
 *   partials : float[4 * stride], row r (0 mse, 1 edge A, 2 edge B, 3 kl) at partials + r * stride.  Every workgroup of a
 *              launch STORES its partial into its own cell (zeros included): no clearing, no atomics;
 *   stride   : capacity of a row, at least the family's *_fwd_partials(...) for the same arguments (host-only queries: the
 *              most workgroups a launch of the family has; `aligned16`: every tensor is 16-byte aligned, which selects the
 *              vector kernels -- accepted and IGNORED by the wide query, whose grids do not depend on alignment; -1 for bad
 *              sizes; the fused query returns -2 where the fused entry does).  A buffer that is too small is an argument
 *              error and nothing is enqueued;
 *   counts   : int32[4] in HOST memory, written by the entry: the number of cells of row r that the launches write
 *              (0: the row is not part of this evaluation -- no 'kl', no edges).
 * The same kernels as the default mode's, instantiated with a store in place of the atomic; R / P / D / stats are bit for bit
 * the default mode's, so every backward entry is used unchanged.  advchain_consistency_lp_fwd_ord covers the lp entry
 * (class_w == NULL) and the cw entry.  advchain_consistency_finish_ord adds row r's counts[r] cells in a fixed order (lane j of
 * one wave takes cells j, j + 64, ...; then a fixed tree) into sums[r] and forms value = sum_r coef[r] * sums[r] with the
 * expression of advchain_consistency_finish.  They work whatever advchain_get_deterministic() says.                    */
int64_t advchain_consistency_fwd_partials(int64_t N, int64_t K, int ndim, const int64_t* dims, int mask_channels, int want_edges,
                                          int aligned16);
int advchain_consistency_fwd_ord(const float* pred, const float* ref, const float* mask, float* P, float* D, float* R,
                                 float* partials, int64_t stride, int32_t* counts, int64_t N, int64_t K, int ndim,
                                 const int64_t* dims, int mask_channels, int ref_is_prob, int want_edges, int want_kl, void* stream);
int64_t advchain_consistency_fused_fwd_partials(int64_t N, int64_t K, int ndim, const int64_t* dims, int has_mask, int mask_channels,
                                                int want_edges, int aligned16);
int advchain_consistency_fused_fwd_ord(const float* pred, const float* ref, const float* mask, float* R, float* partials,
                                       int64_t stride, int32_t* counts, int64_t N, int64_t K, int ndim, const int64_t* dims,
                                       int mask_channels, int ref_is_prob, int want_edges, int want_kl, void* stream);
int64_t advchain_consistency_wide_fwd_partials(int64_t N, int64_t K, int ndim, const int64_t* dims, int want_edges, int aligned16);
int advchain_consistency_wide_fwd_ord(const float* pred, const float* ref, const float* mask, float* stats, float* R,
                                      float* partials, int64_t stride, int32_t* counts, int64_t N, int64_t K, int ndim,
                                      const int64_t* dims, int mask_channels, int ref_is_prob, int want_edges, int want_kl,
                                      void* stream);
int64_t advchain_consistency_lp_fwd_partials(int64_t N, int64_t K, int ndim, const int64_t* dims, int want_edges);
int advchain_consistency_lp_fwd_ord(const void* pred, int pred_bf16, const void* ref, int ref_bf16, const float* mask, float* stats,
                                    float* R, float* partials, int64_t stride, int32_t* counts, int64_t N, int64_t K, int ndim,
                                    const int64_t* dims, int mask_channels, int ref_is_prob, int want_edges, int want_kl,
                                    const float* class_w /*nullable*/, void* stream);
int advchain_consistency_finish_ord(const float* partials, int64_t stride, const int32_t* counts4_host, const float* coef4_host,
                                    float* sums, float* value, void* stream);

/* bf16 STORAGE experiment (round 6; BASELINE config 2 names "bf16"): the 2D K = 4 fused loss above (common/loss.py:8-87,
 * 102-220: mse + contour terms on logits) with pred / ref / R / grad_pred stored as bfloat16 (raw 16-bit words, 8-byte aligned)
 * and all arithmetic in fp32 registers.  NOT used by the product path -- the parity contract is fp32 at 1e-4; the entries exist
 * so that "what would half the bytes buy" is a measurement (tools/kernel_bench.py).  mask: fp32, one
 * channel or NULL.  ADVCHAIN_ERR_UNSUPPORTED (-2) for anything but ndim == 2, K == 4, rows of 4j <= 256 pixels. */
int advchain_consistency_fused_fwd_bf16(const void* pred, const void* ref, const float* mask, void* R, float* sums, int64_t N,
                                        int64_t K, int ndim, const int64_t* dims, void* stream);
int advchain_consistency_fused_bwd_bf16(const void* pred, const void* ref, const void* R, const float* mask,
                                        const float* grad_scale, void* grad_pred, float c_mse, float c_a, float c_b, int64_t N,
                                        int64_t K, int ndim, const int64_t* dims, void* stream);

/* ---- supervised segmentation losses (seg_loss.hip) ---------------------------------------------------------------------
 * Caller-provided workspace of every forward below: advchain_seg_loss_workspace(N, ndim, dims) floats (one partial per
 * workgroup); the value is their fixed-order sum over one more workgroup -- no float atomics, bitwise reproducible.
 * Labels are int64 and only ever compared with class indices (never used as an address).  Returns -1 for bad sizes.      */
int64_t advchain_seg_loss_workspace(int64_t N, int ndim, const int64_t* dims); /* floats */
/* replaces: cross_entropy_2D, advchain/common/loss.py:274-326 (F.log_softmax + F.nll_loss(weight, reduction="none") + sum, or
 *           the soft-target sum -sum_c w_c t_c log p_c).  logits (N,K,H,W) fp32 (logits_bf16 = 0) or bf16 (1, raw 16-bit words);
 *           exactly one of labels (N,H,W) int64 -- -100 contributes 0, any other label outside [0,K) gives NaN -- and soft
 *           (N,K,H,W) fp32; weight (K floats, device) or NULL, used as weight / sum(weight) * K; dims = (H, W).
 *           value[0] = sum over pixels / denom (N*H*W for size_average, else 1).  lse (N*H*W floats: the log-sum-exp per pixel,
 *           kept for the backward) may be NULL.                                                                               */
int advchain_ce2d_fwd(const void* logits, int logits_bf16, const int64_t* labels, const float* soft, const float* weight,
                      float* lse, float* workspace, float* value, int64_t N, int64_t K, const int64_t* dims, float denom,
                      void* stream);
/* replaces: the autograd of the call above.  grad_logits (the logits' dtype) = gs / denom (W p_c - w_c t_c) with W = sum_c w_c t_c;
 *           grad_soft (fp32, soft targets only) = gs / denom * w_c (lse - x_c); either may be NULL (not both);
 *           gs = *grad_scale (device scalar, NULL = 1).                                                                        */
int advchain_ce2d_bwd(const void* logits, int logits_bf16, const int64_t* labels, const float* soft, const float* weight,
                      const float* lse, const float* grad_scale, void* grad_logits, float* grad_soft, int64_t N, int64_t K,
                      const int64_t* dims, float denom, void* stream);
/* replaces: contour_loss, advchain/common/loss.py:102-220 (One_Hot of the labels, the Sobel convolutions of the prediction and
 *           of the target, mask, MSE).  The reference's filters sum over the class axis (Q14), so the loss is the edge energy of
 *           u = sum_{c >= first_class} (input_c - T_c):  2D 1/2 [mean(w (Sx*u)^2) + mean(w (Sy*u)^2)],
 *           3D 1/3 [2 mean(w (A*u)^2) + mean(w (B*u)^2)] (A, B as for advchain_consistency_fwd), means over N * voxels,
 *           w = mean of m^2 over the first min(K - first_class, mask_channels) channels of mask (N, mask_channels, dims) or 1
 *           (mask NULL; in 2D mask_channels must be 1 or >= K - first_class).  input (N,K,dims) fp32; exactly one of labels
 *           (N,dims) int64 (T = one-hot; a label outside [0,K) gives NaN) and soft (N,K,dims) fp32; first_class = 1 when
 *           ignore_background.  R (N,2,dims) = the edge fields weighted for the backward, NULL when none is needed.          */
int advchain_contour_fwd(const float* input, const int64_t* labels, const float* soft, const float* mask, float* R,
                         float* workspace, float* value, int64_t N, int64_t K, int ndim, const int64_t* dims, int first_class,
                         int mask_channels, void* stream);
/* replaces: the autograd of the call above: grad_input_c = g_u, grad_soft_c = -g_u for c >= first_class, 0 for the other
 *           class (both (N,K,dims), either may be NULL, not both), g_u = gs / (N * voxels) * adjoint stencils of R.         */
int advchain_contour_bwd(const float* R, const float* grad_scale, float* grad_input, float* grad_soft, int64_t N, int64_t K,
                         int ndim, const int64_t* dims, int first_class, void* stream);
/* replaces: One_Hot(depth).forward, advchain/common/loss.py:252-271 (eye(depth).index_select + permute): labels (N, V) int64 ->
 *           out (N, depth, V) fp32, planar; a label outside [0, depth) gives a NaN column.                                   */
int advchain_one_hot(const int64_t* labels, float* out, int64_t N, int64_t depth, int64_t V, void* stream);

/* ---- soft Dice and fused Dice + cross entropy, 2D and 3D (seg_dice.hip) ---------------------------------------------------
 * Not in the reference.  logits (N,K,dims) fp32 (logits_bf16 = 0) or bf16 (1, raw 16-bit words), ndim = 2 or 3, 1 <= K <= 65535,
 * N <= 65535; exactly one of labels (N,dims) int64 and soft (N,K,dims) fp32; p = softmax over K, inside the kernel.  A voxel
 * labelled -100 is left out of every Dice sum; any other label outside [0,K) makes the value NaN (labels are only compared
 * with class indices).  Over the counted voxels of entry n (with ADVCHAIN_DICE_BATCH over every entry, N -> 1 below):
 *   I_nk = sum p_k t_k, P_nk = sum p_k, T_nk = sum t_k, D_nk = P_nk + T_nk + smooth, dice_nk = (2 I_nk + smooth) / D_nk,
 *   value = dice_w (1 - 1/N sum_nk omega_k dice_nk) + ce_w CE,   omega_k = w_k / sum of the counted w_j
 * with w = weight (K floats, device) or 1, class 0 not counted under ADVCHAIN_DICE_IGNORE_BACKGROUND, and CE the cross entropy
 * of advchain_ce2d_fwd with denom = N * voxels (weight / sum(weight) * K; -100 contributes 0).  ce_w == 0: pure Dice, no CE
 * work.  smooth == 0 with a class empty on both sides gives NaN.  Per-workgroup partials go to `workspace`
 * (advchain_dice_workspace floats, 16-byte aligned; host-only query, -1 for bad sizes; no clearing needed) and are added in
 * a fixed order: no float atomics, no host read-back, every output written by a kernel -- bitwise reproducible, capturable.
 * Three launches.  lse (N*voxels floats: log-sum-exp per voxel) and coef (N*K*2 floats: A_nk = -2 c omega_k / D_nk,
 * B_nk = c omega_k (2 I_nk + smooth) / D_nk^2, c = 1/N or 1 for batch Dice) are kept for the backward; either may be NULL. */
#define ADVCHAIN_DICE_IGNORE_BACKGROUND 1
#define ADVCHAIN_DICE_BATCH 2
int64_t advchain_dice_workspace(int64_t N, int64_t K, int ndim, const int64_t* dims); /* floats */
int advchain_dice_fwd(const void* logits, int logits_bf16, const int64_t* labels, const float* soft, const float* weight,
                      float* lse, float* coef, float* workspace, float* value, int64_t N, int64_t K, int ndim,
                      const int64_t* dims, int flags, float smooth, float dice_w, float ce_w, void* stream);
/* its gradient, one launch: with g_k = A_nk t_k + B_nk, grad_logits_k = gs [dice_w p_k (g_k - sum_j g_j p_j) + ce_w CE'] (the
 *           logits' dtype, computed in fp32 and rounded once; the Dice part is zero at ignored voxels) and, for a soft target,
 *           grad_soft_k = gs [dice_w (A_nk p_k + B_nk) + ce_w / (N voxels) w_k (lse - x_k)] (fp32); either may be NULL (not
 *           both); gs = *grad_scale (device scalar, NULL = 1); dice_w, ce_w as in the forward.                              */
int advchain_dice_bwd(const void* logits, int logits_bf16, const int64_t* labels, const float* soft, const float* weight,
                      const float* lse, const float* coef, const float* grad_scale, void* grad_logits, float* grad_soft,
                      int64_t N, int64_t K, int ndim, const int64_t* dims, float dice_w, float ce_w, void* stream);

/* ---- soft skeletons and the soft-clDice loss, 2D and 3D (seg_skeleton.hip) -------------------------------------------------
 * Not in the reference (Shit et al., clDice, CVPR 2021).  On every plane of maps (N,K,dims) fp32, with E the minimum over a
 * voxel and its in-image face neighbours and D the maximum over the in-image 3x3(x3) box:
 *   x_0 = x, x_{j+1} = E(x_j), delta_j = relu(x_j - D(x_{j+1})), skel_0 = delta_0,
 *   skel_j = skel_{j-1} + relu(delta_j - skel_{j-1} delta_j),  j = 1..iterations (0..ADVCHAIN_SKELETON_MAX_ITERATIONS),
 * each operation rounded once in fp32: the bits of the published max_pool composition.  route: ADVCHAIN_SKELETON_AUTO, _FUSED
 * (one launch, the chain of a tile with a halo of iterations + 2 in LDS; at most ADVCHAIN_SKELETON_FUSED_MAX iterations, an
 * error beyond) or _LEVELS (iterations + 2 launches, any count); the same bits on both.  `workspace`: advchain_skeleton_workspace
 * floats for `what` = 0 (soft_skeleton_fwd), 1 (soft_skeleton_bwd), 2 (cldice_fwd), 3 (cldice_bwd), 16-byte aligned, no clearing
 * needed; a host-only query, -1 for bad sizes.  No float atomics, no memset, no host read-back: bitwise reproducible,
 * capturable on one stream.                                                                                                  */
#define ADVCHAIN_SKELETON_MAX_ITERATIONS 32
#define ADVCHAIN_SKELETON_FUSED_MAX 4
#define ADVCHAIN_SKELETON_AUTO 0
#define ADVCHAIN_SKELETON_FUSED 1
#define ADVCHAIN_SKELETON_LEVELS 2
int64_t advchain_skeleton_workspace(int64_t N, int64_t K, int ndim, const int64_t* dims, int iterations, int what); /* floats */
int advchain_soft_skeleton_fwd(const float* maps, float* skeleton, float* workspace, int64_t N, int64_t K, int ndim,
                               const int64_t* dims, int iterations, int route, void* stream);
/* its gradient, in gather form (the erosion chain is recomputed into the workspace with a 1-byte selection code per voxel and
 *           level; 2 iterations + 4 launches): grad_maps (N,K,dims) from grad_skeleton (N,K,dims).  relu'(0) = 0; among equal
 *           window values the first wins: centre, then axis by axis, minus before plus (E); centre, then raster order (D).     */
int advchain_soft_skeleton_bwd(const float* maps, const float* grad_skeleton, float* grad_maps, float* workspace, int64_t N,
                               int64_t K, int ndim, const int64_t* dims, int iterations, void* stream);
/* soft-clDice of logits (N,K,dims) fp32 / bf16 against labels (N,dims) int64 or a soft target (N,K,dims) fp32 (exactly one):
 *   p = softmax over K (inside the kernels), t = one-hot (a label outside [0,K), -100 included: no class), m = 0 at -100,
 *   S^p = skel(p), S^t = skel(t);  over the voxels of entry n (ADVCHAIN_DICE_BATCH: of every entry, N -> 1)
 *   Tprec = (sum m S^p t + smooth) / (sum m S^p + smooth),  Tsens = (sum m S^t p + smooth) / (sum m S^t + smooth),
 *   value = 1 - 1/rows sum_nk omega_k 2 Tprec Tsens / (Tprec + Tsens),   omega_k = w_k / sum of the counted w_j
 * (flags as advchain_dice_fwd).  lse (N*voxels), skeleton_target (N*K*voxels) and coef (N*K*3: dL/dS^p = m (A t + B), the
 * direct dL/dp = m C S^t) are kept for the backward; coef may be NULL.                                                      */
int advchain_cldice_fwd(const void* logits, int logits_bf16, const int64_t* labels, const float* soft, const float* weight,
                        float* lse, float* skeleton_target, float* coef, float* workspace, float* value, int64_t N, int64_t K,
                        int ndim, const int64_t* dims, int iterations, int route, int flags, float smooth, void* stream);
/* its gradient for the logits (their dtype, computed in fp32 and rounded once); gs = *grad_scale (device scalar, NULL = 1). */
int advchain_cldice_bwd(const void* logits, int logits_bf16, const int64_t* labels, const float* soft, const float* lse,
                        const float* skeleton_target, const float* coef, const float* grad_scale, void* grad_logits,
                        float* workspace, int64_t N, int64_t K, int ndim, const int64_t* dims, int iterations, void* stream);

/* ---- Euclidean distance transform and signed distance maps, 2D and 3D (edt.hip) --------------------------------------------
 * Not in the reference.  Exact and separable: one pass along the contiguous axis (both sides of every row), then per further
 * axis the lower envelope min_j f(j) + (s (i - j))^2 from LDS-staged lines.  `dims` is (H, W) or (D, H, W); `sampling` is NULL
 * (unit spacing: int32 squared distances, exact, the same bits on every run) or ndim positive finite HOST floats in the order
 * of dims (fp32 fields, no contraction).  ADVCHAIN_ERR_UNSUPPORTED for a shape the fields cannot hold: an axis above 32767, a
 * squared diagonal of 2^30 or more (the "no seed yet" sentinel: sentinel + offset^2 stays below 2^31), or one of the
 * non-contiguous axes above 16384 (8192 for the signed maps: one x of a whole line, of both fields, is staged in 64 KiB of LDS).
 * No atomics, no memset, no host read-back; capturable on one stream.
 * advchain_edt: mask (B, dims), mask_kind 1 = 8-bit (bool / uint8), 2 = int64, 3 = fp32; nonzero is foreground (NaN too).
 *           out (B, dims) fp32: at a foreground voxel the Euclidean distance (squared = 1: its square, with unit spacing an
 *           exact integer up to 2^24) to the nearest zero voxel of the same entry b, 0 at a zero voxel -- scipy's
 *           distance_transform_edt -- and +inf at the foreground voxels of an entry without a zero voxel.  `out` doubles as
 *           the field between the passes: no workspace.                                                                     */
int advchain_edt(const void* mask, int mask_kind, const float* sampling, int squared, float* out, int64_t B, int ndim,
                 const int64_t* dims, void* stream);
/* advchain_signed_maps: labels (N, dims) int64 -> out (N, K, dims) fp32, straight from the labels (no one-hot tensor):
 *           phi_nk(v) = d(v, F_nk) - d(v, B_nk), F_nk = {u: labels[n,u] == k}, B_nk its complement in entry n: positive outside
 *           the class, negative inside, at least one spacing in magnitude (the symmetric convention; Kervadec's one_hot2dist
 *           has (d(v, B) - 1) inside).  A label outside [0, K), -100 included, belongs to no class; labels are only compared
 *           with class indices.  A class absent from entry n, or filling it, has no boundary: its plane is 0.  Both fields
 *           of every (n, k) -- squared distance to the nearest member and to the nearest non-member -- go through the passes in
 *           `workspace` (advchain_signed_maps_workspace 4-byte words, 16-byte aligned; host-only query, -1 for bad sizes; no
 *           clearing needed); the last pass evaluates only the field that the voxel's own membership selects.              */
int64_t advchain_signed_maps_workspace(int64_t N, int64_t K, int ndim, const int64_t* dims); /* floats */
int advchain_signed_maps(const int64_t* labels, const float* sampling, float* out, float* workspace, int64_t N, int64_t K,
                         int ndim, const int64_t* dims, void* stream);

/* ---- surface distance metrics of a pair of label maps, 2D and 3D (seg_surface.hip) -------------------------------------------
 * Not in the reference.  pred, target (N, dims) int64; for entry n and class k, A = {v: pred[n,v] == k}, B = {v: target[n,v] ==
 * k}; a label outside [0, K), -100 included, belongs to no class, and labels are only compared with class indices.  The border
 * dS of a set is its voxels with a face neighbour (4 in 2D, 6 in 3D) outside it, a position outside the image counting as
 * outside (S ^ binary_erosion(S)).  Direction 0 is the multiset {d(a, dB): a in dA} of size m0, direction 1 {d(b, dA): b in dB}
 * of size m1, d the Euclidean distance under `sampling` (as for the transform above: NULL, or ndim host floats).  Per direction
 * the maximum, the mean, and the percentile q in [0, 100] by numpy's linear rule: h = (m - 1) (q / 100), j = floor(h),
 * P = x_(j) + (h - j) (x_(min(j+1, m-1)) - x_(j)) over the sorted distances, in fp64.  Outputs (all written, device memory):
 *   hausdorff (N,K) fp32       max of the two maxima
 *   hausdorff_pct (N,K) fp32   max of the two percentiles (not the percentile of the pooled distances)
 *   assd (N,K) fp32            (sum0 + sum1) / (m0 + m1)
 *   directed (N,K,2,3) fp32    direction x (maximum, percentile, mean)
 *   surface_voxels (N,K,2) int64   m0, m1
 *   max_squared (N,K,2) fp64   the largest squared distance per direction, an exact integer with unit spacing
 *   overlap (N,K,3) int64      |A|, |B|, |A n B|
 *   dice (N,K) fp32            2 |A n B| / (|A| + |B|), NaN when both are empty
 * Both borders empty: every distance of (n, k) is NaN; exactly one empty: +inf.  With unit spacing the squared distances are
 * int32 and exact, roots, interpolation and means are taken in fp64 and rounded to fp32 once.  One pass writes the two edge
 * label maps (int64: the label at a border voxel, -1 elsewhere) and the counts; the passes of the transform give the squared
 * distance of every voxel to the nearest border voxel of each class of each map; a border voxel then contributes one field word,
 * and a four-digit radix select (LDS histograms, 64-bit integer atomics) finds the order statistics.  Sums are fp64 partials
 * per workgroup added in a fixed order.  Integer atomics only, no memset, no host read-back: bitwise reproducible, capturable
 * on one stream.  ADVCHAIN_ERR_UNSUPPORTED for the shapes advchain_signed_maps refuses, and for N above 65535.
 * `workspace` (16-byte aligned, no clearing needed): advchain_surface_metrics_workspace 4-byte words, host-only query, -1 where
 * the shape is refused; with V voxels per entry and c = min(ceil(V / 4096), 256) it is
 *   2 N K V (fields) + 4 N V (edge maps) + 2 N K (512 + 2 + 2 c + 4) (histograms, ranks, partial sums, segment words).        */
int64_t advchain_surface_metrics_workspace(int64_t N, int64_t K, int ndim, const int64_t* dims); /* 4-byte words */
int advchain_surface_metrics(const int64_t* pred, const int64_t* target, const float* sampling, double q, float* hausdorff,
                             float* hausdorff_pct, float* assd, float* directed, int64_t* surface_voxels, double* max_squared,
                             int64_t* overlap, float* dice, void* workspace, int64_t N, int64_t K, int ndim,
                             const int64_t* dims, void* stream);

/* ---- surface Dice at a tolerance (NSD) of a pair of label maps, 2D and 3D (seg_surface.hip) -----------------------------------
 * Not in the reference; MONAI's compute_surface_dice (voxel counts, not surface areas).  pred, target, A, B, the border dS, the
 * directions and `sampling` as for advchain_surface_metrics above.  With a tolerance tau_k per class:
 *   within (N,K,2) int64          c0 = #{a in dA: d(a, dB) <= tau_k}, c1 = #{b in dB: d(b, dA) <= tau_k}
 *   surface_voxels (N,K,2) int64  m0 = |dA|, m1 = |dB| (the integers of advchain_surface_metrics)
 *   surface_dice (N,K) fp32       (c0 + c1) / (m0 + m1) in fp64, rounded once; NaN when m0 + m1 == 0; 0 when exactly one border is
 *                                 empty (every distance is +inf: nothing is within)
 * `thresholds`: K 32-bit words in DEVICE memory, the squared tolerances as the comparison takes them (the ball rule of
 * advchain_morph).  sampling NULL: int32 T_k = min(floor(tau_k^2), 2^30 - 1) and the test d^2 <= T_k is on exact integers
 * (tau = 2 includes the squared length 4; sqrt(3) in double gives T = 2).  With a sampling: the bits of tau_k^2 rounded to fp32
 * once (at most 1e29), compared with the fp32 squared distance of the transform, ((s_x dx)^2 + (s_y dy)^2) + (s_z dz)^2 without
 * contraction: a tolerance equal to a multiple of the spacing can fall on either side.  `tolerance_max` (host): the largest
 * tau_k; it bounds the search and chooses the route.  Two routes, equal bits:
 *   1 "ball"    one kernel stages a tile of both maps with a halo of cap_a + 1 voxels in LDS, cap_a = min(floor(tau_max / s_a),
 *               dims_a - 1), and every border voxel looks for a border voxel of its class of the other map inside the ball; cost
 *               independent of K, no workspace.  Eligible iff K <= 65534 and a tile of (32,64) (16,64) (8,64) in 2D, (8,8,32)
 *               (4,8,32) (4,4,32) (2,4,32) (2,2,32) in 3D with that halo, at 5 bytes a cell, fits 60 KiB of LDS.
 *   2 "fields"  the edge pass and distance fields of advchain_surface_metrics, then one count pass key <= threshold; any
 *               tolerance, the shape limits of advchain_surface_metrics.
 * `route`: 0 dispatch (the ball where it is eligible and no cap exceeds 5 in 2D, 2 in 3D -- where it was measured to be the
 * faster one -- else the fields, else the ball), 1 or 2 forces one.
 * advchain_surface_dice_route: the route a call takes (1 or 2), host-only; ADVCHAIN_ERR_UNSUPPORTED where none can (a forced
 * ball that is not eligible; a shape the fields refuse).  advchain_surface_dice_workspace: 4-byte words of `workspace` for that
 * route (16-byte aligned, no clearing needed; 0 for the ball: `workspace` may be NULL), -1 where the call would be refused:
 *   fields: 2 N K V + 4 N V + 6 N K.
 * Integer atomics only, no memset, no host read-back: bitwise reproducible, capturable on one stream.                          */
int advchain_surface_dice_route(int64_t N, int64_t K, int ndim, const int64_t* dims, const float* sampling, double tolerance_max,
                                int route);
int64_t advchain_surface_dice_workspace(int64_t N, int64_t K, int ndim, const int64_t* dims, const float* sampling,
                                        double tolerance_max, int route); /* 4-byte words */
int advchain_surface_dice(const int64_t* pred, const int64_t* target, const float* sampling, const void* thresholds,
                          double tolerance_max, int route, float* surface_dice, int64_t* within, int64_t* surface_voxels,
                          void* workspace, int64_t N, int64_t K, int ndim, const int64_t* dims, void* stream);

/* ---- connected components of label maps and the filters on them, 2D and 3D (seg_components.hip) -----------------------------
 * Not in the reference.  labels (N, dims) int64, dims = (H, W) or (D, H, W).  Two voxels of an entry are adjacent when their
 * offsets differ by at most 1 on every axis and on at most `connectivity` axes (1 .. ndim: scipy's generate_binary_structure);
 * adjacent voxels are connected when they carry the same label and that label is foreground: not `background` and, with
 * num_classes >= 0, inside [0, num_classes) (-100 is then background; a negative num_classes means no class count).  Labels are
 * only compared; keep_largest alone uses one as an index, after that range check.  Components never span entries.  A
 * label-equivalence union-find: a tile of 2048 voxels is resolved in LDS (each label read once), the tile seams -- edges and
 * corners included -- are united in global memory with a lock-free atomic minimum, every voxel is pointed at its root, the
 * smallest linear index (C order, within the entry) of its component.  Integer atomics only, no workgroup waits on another, no
 * memset, no host read-back: the same bits on every run, capturable on one stream.  ADVCHAIN_ERR_UNSUPPORTED for more than
 * 2^31 - 1 voxels in an entry or a workspace of more than 2^31 - 1 words.
 * `workspace` (no clearing needed): advchain_components_workspace 4-byte words, host-only query, -1 where the shape is refused;
 * with V voxels per entry it is N (2 V + ceil(V / 2048)): parents, sizes, root counts per chunk of 2048 voxels.
 * advchain_components: out_labels (N, dims) int32: 0 on background, else the number of the voxel's component, 1 .. count[n], the
 *           components of an entry in the order of their smallest linear index; count (N) int64; sizes (N, dims) int32 or NULL:
 *           the voxel count of the component of each voxel, 0 on background.                                                 */
int64_t advchain_components_workspace(int64_t N, int ndim, const int64_t* dims); /* 4-byte words */
int advchain_components(const int64_t* labels, int32_t* out_labels, int64_t* count, int32_t* sizes, void* workspace, int64_t N,
                        int ndim, const int64_t* dims, int connectivity, int64_t background, int64_t num_classes, void* stream);
/* advchain_keep_largest: out (N, dims) int64, not the input: for every entry and class k in [0, K) other than `background`, a voxel
 *           of class k outside the largest component of class k of its entry becomes `background`; ties go to the component
 *           with the smaller smallest linear index (one 64-bit atomic maximum of (size << 32) | (2^32 - 1 - root) per class);
 *           every other voxel, labels outside [0, K) included, is copied.  `winners`: N K 8-byte words, 8-byte aligned, no
 *           clearing needed.  K in 1 .. 65535.                                                                              */
int advchain_keep_largest(const int64_t* labels, int64_t* out, void* workspace, void* winners, int64_t N, int64_t K, int ndim,
                          const int64_t* dims, int connectivity, int64_t background, void* stream);
/* advchain_remove_small: out (N, dims) int64, not the input: the voxels of components of fewer than min_size (>= 1) voxels become
 *           `background`, every other voxel is copied -- also a label that num_classes makes background: it is in no component. */
int advchain_remove_small(const int64_t* labels, int64_t* out, void* workspace, int64_t N, int ndim, const int64_t* dims,
                          int connectivity, int64_t background, int64_t num_classes, int64_t min_size, void* stream);
/* advchain_fill_holes: the same passes label the BACKGROUND: a background component is a class of the transitive closure of
 *           "adjacent under `connectivity` and both equal to `background`" within an entry.  It touches the border when one of
 *           its voxels has a coordinate 0 or size - 1 on a spatial axis; its enclosing labels are those of the voxels adjacent
 *           (same connectivity) to one of its voxels that are not `background`.  A hole is a background component that does not
 *           touch the border, whose enclosing labels are all one value k in [0, K), and, with max_size >= 1, that has at most
 *           max_size voxels (max_size < 0: no limit; 0 is refused).  A component enclosed by two labels, or adjacent to a label
 *           outside [0, K), stays.  out (N, dims) int64 or NULL: the input with the voxels of every hole set to its k, every
 *           other voxel copied; fill (N, dims) int64 or NULL: k on the voxels of a hole, -1 elsewhere; neither is the input.
 *           count, voxels (N, K) int64, 8-byte aligned, NULL together, no clearing needed: the holes filled and their voxels
 *           per entry and enclosing class.  At least one output.  K in 1 .. 65535.  Per root a smallest and a largest enclosing
 *           code kept by integer atomic minimum and maximum, one turn per distinct root of a wave.
 * `workspace`: advchain_fill_holes_workspace 4-byte words, -1 exactly where advchain_components_workspace is: that workspace
 *           and 2 N V words of enclosure state.                                                                               */
int64_t advchain_fill_holes_workspace(int64_t N, int ndim, const int64_t* dims); /* 4-byte words */
int advchain_fill_holes(const int64_t* labels, int64_t* out, int64_t* fill, int64_t* count, int64_t* voxels, void* workspace,
                        int64_t N, int64_t K, int ndim, const int64_t* dims, int connectivity, int64_t background,
                        int64_t max_size, void* stream);
/* advchain_instance_match: instance-wise detection metrics of a pair of label maps (F1 / recognition quality, segmentation and
 *           panoptic quality).  pred and target (N, dims) int64 are labelled by the passes above with num_classes = K, each into
 *           its own part of the workspace.  Per entry n and class k: P and T are the components of class k of pred[n] and
 *           target[n], nP = |P|, nT = |T|; for a in P and b in T, I = |a n b| and U = |a| + |b| - I; the pair overlaps when
 *           I >= 1 and matches when (double)I > iou_threshold * (double)U (one fp64 product, one comparison).  iou_threshold in
 *           [0.5, 1): with the strict inequality a component matches at most one partner, so the matches are a matching and no
 *           assignment step exists.  Outputs, none needs clearing:
 *             components (N,K,2) int64   nP, nT
 *             matched (N,K) int64        TP, the number of matches (FP = nP - TP, FN = nT - TP)
 *             overlapping (N,K,2) int64  components of P that overlap at least one of T, and of T that overlap at least one of P
 *             iou_fixed (N,K) int64      the sum over the matches of (I << 32) / U in unsigned 64-bit integers: exact, below 2^63
 *             precision, recall, f1, sq, pq (N,K) fp32   TP / nP, TP / nT, 2 TP / (nP + nT), S / TP, 2 S / (nP + nT) with
 *                                        S = (double)iou_fixed 2^-32, each one fp64 division rounded to fp32 once; NaN when the
 *                                        denominator is 0.  The row of k == background is zeros and NaN.
 *             pred_status, target_status (N, dims) uint8 or NULL ("not wanted"): 0 in no component, 1 its component is matched,
 *                                        2 unmatched but overlapping a component of its class of the other map, 3 overlapping none
 *           The overlaps are counted in an open-addressing table per entry (64-bit keys (root in pred << 32) | root in target
 *           claimed by compare-and-swap, linear probing, integer adds; a wave adds once per run of equal keys) of max(2 V, 64)
 *           slots: an entry has at most V distinct pairs, so an empty slot always exists and nothing overflows.  K in 1 .. 65535.
 *           Integer atomics only, no memset, no host read-back: the same bits on every run, capturable on one stream.
 * `workspace` (8-byte aligned, no clearing needed): advchain_instance_match_workspace 4-byte words, host-only query, -1 where
 *           advchain_components_workspace is or for more than 2^31 - 1 words; with V voxels per entry and S = max(2 V, 64) it is
 *           N (3 S + 6 V + 2 ceil(V / 2048)): the table, a state word per voxel and map, two labelling workspaces.           */
int64_t advchain_instance_match_workspace(int64_t N, int ndim, const int64_t* dims); /* 4-byte words */
int advchain_instance_match(const int64_t* pred, const int64_t* target, int64_t* components, int64_t* matched,
                            int64_t* overlapping, int64_t* iou_fixed, float* precision, float* recall, float* f1, float* sq,
                            float* pq, uint8_t* pred_status, uint8_t* target_status, void* workspace, int64_t N, int64_t K,
                            int ndim, const int64_t* dims, int connectivity, int64_t background, double iou_threshold,
                            void* stream);
/* advchain_betti: Betti numbers, Euler characteristic and Betti error of label maps.  pred and target (N, dims) int64; target may
 *           be NULL (one map: M = 1), else M = 2 and map 0 is pred.  Per entry n and class k, for EVERY k in [0, K) (there is no
 *           background): A = {v : label == k}; a label outside [0, K) is in no class and in the complement of every class;
 *           positions outside the image are in no class.  `connectivity` c is the adjacency of A, its complement gets the dual
 *           one: 2D c = 1: 4 and 8, c = 2: 8 and 4; 3D c = 1: 6 and 26, c = 3: 26 and 6; c = 2 in 3D (18) has no dual and is
 *           refused (ADVCHAIN_ERR_ARG).  chi: the Euler characteristic of the cubical complex of A -- c = ndim: voxels are
 *           closed cubes: vertices - edges + faces - cubes; c = 1: the dual complex: voxels - face pairs + 2x2 squares - 2x2x2
 *           blocks that lie in A -- summed over the windows of the lattice corners in integers.  b0: the components of A under c.
 *           cav: the components of the complement under the dual adjacency that hold no voxel with a coordinate 0 or size - 1.
 *           2D: b1 = b0 - chi, b2 = 0.  3D: b2 = cav, b1 = b0 + b2 - chi.  Outputs, 8-byte aligned, none needs clearing:
 *             betti (N,K,M,3) int64   b0, b1, b2
 *             euler (N,K,M) int64     chi
 *             error (N,K,3) int64 or NULL (only with a target)   |b_i(pred) - b_i(target)|
 *           One labelling of all classes and one pass over the windows per map; in 3D one more labelling per class and map for
 *           the cavities (1 + K in all), through the same workspace.  Sums per class are taken in LDS up to 2048 classes and
 *           with global 64-bit integer atomics above.  K in 1 .. 65535.  Integer atomics only, no memset, no host read-back: the
 *           same bits on every run, capturable on one stream.
 * `workspace`: advchain_betti_workspace 4-byte words, host-only query: advchain_components_workspace, whatever K and M are.    */
int64_t advchain_betti_workspace(int64_t N, int ndim, const int64_t* dims); /* 4-byte words */
int advchain_betti(const int64_t* pred, const int64_t* target, int64_t* betti, int64_t* euler, int64_t* error, void* workspace,
                   int64_t N, int64_t K, int ndim, const int64_t* dims, int connectivity, void* stream);

/* ---- confusion matrix and per-class overlap scores, also from logits, 2D and 3D (seg_confusion.hip) ---------------------------
 * Not in the reference.  target (N, dims) int64, dims = (H, W) or (D, H, W).  `pred_kind` says what pred is: 0 an int64 label map
 * (N, dims); 1 fp32 or 2 bf16 logits or probabilities (N, K, dims), whose argmax over the class axis is the prediction: the first
 * maximal class wins, a NaN is larger than everything (the first NaN wins), a row of -inf gives class 0 -- torch.argmax on the
 * CPU; bf16 is widened to fp32, exactly.  A_k = {v : pred[v] == k}, B_k = {v : target[v] == k} for every k in [0, K); a label
 * outside [0, K) is in no class and is never used as an address.  With has_ignore = 1 a voxel whose TARGET equals ignore_index is
 * left out of every count (has_ignore = 0: nothing is left out, whatever ignore_index holds).  labels_out (N, dims) int64 or NULL:
 * the argmax map, written in the same pass (logits only).  `flags`: 1 reduce_batch -- the outputs lose their leading N and every
 * entry adds into the same counters; 2 accumulate (advchain_confusion only) -- the counters are not cleared first, the call adds
 * into what they hold.  Outputs, 8-byte aligned; none needs clearing without flag 2:
 *   advchain_confusion       matrix (N,K,K) int64       [n,t,p] = #{counted v : target = t, pred = p}: rows are the truth
 *                            pred_only (N,K) int64      #{counted v : pred = k, target outside [0, K)}
 *                            target_only (N,K) int64    #{counted v : target = k, pred outside [0, K)}
 *                            counted (N) int64          voxels not left out by ignore_index
 *                            K in 1 .. 1024 (8 MB of matrix per entry).
 *   advchain_overlap         overlap (N,K,3) int64      |A|, |B|, |A n B| over the counted voxels; counted (N) int64;
 *                            dice, iou, precision, recall, specificity (N,K) fp32: with TP = |A n B|, FP = |A| - TP,
 *                            FN = |B| - TP, TN = counted - TP - FP - FN: 2 TP / (|A| + |B|), TP / (|A| + |B| - TP), TP / |A|,
 *                            TP / |B|, TN / (TN + FP), each one fp64 division rounded to fp32 once, NaN when the denominator
 *                            is 0.  No matrix is built: 3 K counters per entry, K in 1 .. 65535.
 *   advchain_overlap_scores  the same overlap, counted and quotients from R finished matrices (R,K,K) int64 taken as complete:
 *                            |A_k| the column sum, |B_k| the row sum, TP the diagonal, counted the total.
 * One streaming pass: a lane owns 4 consecutive voxels (16-byte loads where pointers and sizes allow, scalar otherwise: the
 * results do not depend on alignment), a workgroup walks tiles of 1024 voxels of one entry, at most 128 workgroups an entry (more
 * only where a workgroup would otherwise see 2^31 voxels or more).  A wave groups equal keys so that one lane adds a group's
 * count; the adds go to 32-bit counters in LDS (the matrix up to K = 127, overlap up to K = 2048), flushed once with 64-bit
 * global adds, or straight to the global counters above.  Integer atomics only, no memset, no workspace, no host read-back: the
 * same bits on every run, capturable on one stream.  advchain_confusion_limit(what): 0 the voxels of a tile, 1 the cap on
 * workgroups per entry, 2 the largest K of the LDS matrix, 3 the largest K of the matrix, 4 the largest K of the LDS overlap
 * counters; -1 otherwise.  Host only.                                                                                          */
int64_t advchain_confusion_limit(int what);
int advchain_confusion(const void* pred, int pred_kind, const int64_t* target, int64_t* labels_out, int64_t* matrix,
                       int64_t* pred_only, int64_t* target_only, int64_t* counted, int64_t N, int64_t K, int ndim,
                       const int64_t* dims, int has_ignore, int64_t ignore_index, int flags, void* stream);
int advchain_overlap(const void* pred, int pred_kind, const int64_t* target, int64_t* labels_out, int64_t* overlap,
                     int64_t* counted, float* dice, float* iou, float* precision, float* recall, float* specificity, int64_t N,
                     int64_t K, int ndim, const int64_t* dims, int has_ignore, int64_t ignore_index, int flags, void* stream);
int advchain_overlap_scores(const int64_t* matrix, int64_t* overlap, int64_t* counted, float* dice, float* iou, float* precision,
                            float* recall, float* specificity, int64_t R, int64_t K, void* stream);

/* ---- erosion, dilation, opening and closing of label maps with a Euclidean ball, 2D and 3D (seg_morph.hip) ---------------------
 * Not in the reference.  labels (N, dims) int64, dims = (H, W) or (D, H, W); K classes; `background` any integer.  A class voxel
 * carries a label k in [0, K) other than `background`; S_k is the set of voxels of an entry with label k.  A label outside [0, K)
 * (-100, K + 3) is neither class nor background: it is copied, never changes, never grows, and counts as "another label".  Labels
 * are only compared.  Nothing crosses batch entries.  The ball is B = {o : sum_a (s_a o_a)^2 <= radius^2}, s = `sampling` (NULL:
 * 1, and then the test is the integer one, |o|^2 <= floor(radius^2), capped at 2^30 - 1; otherwise ndim host floats, and the test
 * is on fp32 fields against radius^2 rounded to fp32).  A position outside the image is nothing: not a member of any class
 * (dilation gains nothing from it) and not an obstacle (erosion is not eaten from the border): scipy's binary_dilation with
 * border_value=0 and binary_erosion with border_value=1.  `op`:
 *   0 erosion   a class voxel v of class k keeps k iff every in-image v + o, o in B, carries k; otherwise it becomes `background`.
 *   1 dilation  a background voxel becomes the class of the class voxel u within the ball that minimises (|s (v - u)|^2,
 *               labels[u]) lexicographically: nearest wins, among equally near the smaller class.  Classes never overwrite.
 *   2 opening   per class E_k = erosion of S_k, O_k = {v : d^2(v, E_k) <= radius^2}; a class voxel of class k outside O_k becomes
 *               `background`.  Not dilation(erosion(x)), where freed voxels would be contested between classes.
 *   3 closing   per class D_k = {v in the image : d^2(v, S_k) <= radius^2} (voxels of any label), C_k = {v : every in-image v + o
 *               lies in D_k}; a background voxel becomes k iff it lies in C_k for exactly one class k; claimed by two, it stays.
 * Every other voxel is copied.  out (N, dims) int64 is not the input.  A ball that holds only the origin gives a copy.
 * Erosion and dilation run ONE field per voxel whatever K is (the squared distance to the nearest other label; the key
 * (squared distance, class) of the nearest class voxel), every scan bounded at ceil(radius / spacing) offsets; opening and
 * closing take their per-class fields from the passes of the transform above, never for k == background.  No atomics, no
 * memset, no host read-back: the same bits on every run, capturable on one stream.  K in 1 .. 65535; ADVCHAIN_ERR_UNSUPPORTED
 * for the shapes advchain_signed_maps refuses.
 * `workspace` (16-byte aligned, no clearing needed): advchain_morph_workspace 4-byte words, host-only query, -1 for a bad op and
 * exactly where advchain_signed_maps_workspace is -1; with V voxels per entry it is N V (erosion), 2 N V (dilation),
 * N V (2 + K) (opening), N V (2 + K) + ceil(N K V / 4) (closing).                                                              */
int64_t advchain_morph_workspace(int op, int64_t N, int64_t K, int ndim, const int64_t* dims); /* 4-byte words */
int advchain_morph(const int64_t* labels, const float* sampling, double radius, int op, int64_t* out, void* workspace, int64_t N,
                   int64_t K, int64_t background, int ndim, const int64_t* dims, void* stream);

/* ---- boundary (surface) loss, 2D and 3D (seg_boundary.hip) -----------------------------------------------------------------
 * Not in the reference (Kervadec et al.).  logits (N,K,dims) fp32 (logits_bf16 = 0) or bf16 (1), maps (N,K,dims) fp32 signed
 * distance maps (a constant), p = softmax over K inside the kernel:
 *   value = 1/(N voxels) sum_n sum_{v counted} sum_{k counted} omega_k p_k(v) maps_nk(v),  omega_k = w_k / sum of the counted w_j
 * with w = weight (K floats, device) or 1 and class 0 not counted under ADVCHAIN_BOUNDARY_IGNORE_BACKGROUND.  labels (N,dims)
 * int64 or NULL: with labels a voxel labelled -100 is not counted (it stays in N voxels) and any other label outside [0,K)
 * makes value and gradient NaN; with NULL every voxel is counted.  One sweep over logits and maps (online max / sum), one
 * partial per workgroup in `workspace` (advchain_boundary_workspace floats; host-only query, -1 for bad sizes; no clearing
 * needed), added in a fixed order by a second launch: no float atomics, no host read-back, bitwise reproducible, capturable.
 * saved (N,2,voxels floats, or NULL): log-sum-exp and t(v) = sum_k omega_k maps_k p_k per voxel, for the backward.            */
#define ADVCHAIN_BOUNDARY_IGNORE_BACKGROUND 1
int64_t advchain_boundary_workspace(int64_t N, int64_t K, int ndim, const int64_t* dims); /* floats */
int advchain_boundary_fwd(const void* logits, int logits_bf16, const int64_t* labels, const float* maps, const float* weight,
                          float* saved, float* workspace, float* value, int64_t N, int64_t K, int ndim, const int64_t* dims,
                          int flags, void* stream);
/* its gradient, one launch: grad_logits_j = gs / (N voxels) p_j (omega_j maps_j - t) at counted voxels, 0 elsewhere (the logits'
 *           dtype, computed in fp32 and rounded once); gs = *grad_scale (device scalar, NULL = 1).                          */
int advchain_boundary_bwd(const void* logits, int logits_bf16, const int64_t* labels, const float* maps, const float* weight,
                          const float* saved, const float* grad_scale, void* grad_logits, int64_t N, int64_t K, int ndim,
                          const int64_t* dims, int flags, void* stream);

/* ---- deformation helpers (deform_diff.hip) -----------------------------------------------------------------------------
 * The module-level helpers of adv_morph.py that users call to inspect or regularise a deformation.  H and W at least 2 (the
 * reference raises IndexError at 1), N < 65536.  Forwards round once per ATen op of the reference, in its order (no
 * contraction): bit for bit the reference's fp32 values.  Backwards are gathers (no atomics): bitwise reproducible.        */
/* replaces: calculate_image_diff, adv_morph.py:57-77.  in (N,C,H,W) -> dx (along W), dy (along H), both (N,C,H,W): the central
 *           difference 0.5 (v[i+1] - v[i-1]) inside, one-sided differences at the first and last column / row.  12 B/px.     */
int advchain_image_diff2d_fwd(const float* in, float* dx, float* dy, int64_t N, int64_t C, const int64_t* dims, void* stream);
/* replaces: the autograd of the call above: grad_in = Dx^T grad_dx + Dy^T grad_dy; either gradient may be NULL (zero).  12 B/px. */
int advchain_image_diff2d_bwd(const float* grad_dx, const float* grad_dy, float* grad_in, int64_t N, int64_t C,
                              const int64_t* dims, void* stream);
/* replaces: calculate_jacobian_determinant(data, 'displacement'), adv_morph.py:80-100.  field (N,2,H,W) = (u, v) -> det (N,1,H,W)
 *           = (1 + dxx)(1 + dyy) - dxy dyx with (dxx, dxy) = diff(u), (dyx, dyy) = diff(v), per pixel (the reference's units).
 *           12 B/px.                                                                                                          */
int advchain_jacobian_det2d_fwd(const float* field, float* det, int64_t N, const int64_t* dims, void* stream);
/* replaces: its autograd: grad_u = Dx^T(g (1 + dyy)) - Dy^T(g dyx), grad_v = Dy^T(g (1 + dxx)) - Dx^T(g dxy), the derivatives
 *           recomputed from `field` (no saved planes).  grad_field (N,2,H,W).  20 B/px.                                        */
int advchain_jacobian_det2d_bwd(const float* grad_det, const float* field, float* grad_field, int64_t N, const int64_t* dims,
                                void* stream);
/* replaces: get_base_grid + duv / (2.0 ** nb_steps) + integrate_by_add of vectorFieldExponentiation{2,3}D (adv_morph.py:126-130,
 *           153-163): phi0 = identity + duv * inv, inv = 2^-n (exact).  duv, phi0 (N, ndim, dims).                           */
int advchain_expo_start(const float* duv, float* phi0, float inv, int64_t N, int ndim, const int64_t* dims, void* stream);
/* replaces: the torch.norm(duv_interval) of vectorFieldExponentiation3D (adv_morph.py:159), squared and before the 2^-n: out[0] =
 *           sum of x[i]^2 over n values.  One partial per workgroup into `partials` (ADVCHAIN_SUMSQ_PARTIALS floats), then
 *           one workgroup adds them in a fixed order: out[0] is a deterministic function of x.                               */
#define ADVCHAIN_SUMSQ_PARTIALS 1024
int advchain_sumsq_ordered(const float* x, int64_t n, float* partials, float* out, void* stream);

/* ---- Jacobian determinant and folding statistics in 2D and 3D (jacobian.hip) ------------------------------------------------
 * Not in the reference (its helpers assert 2D displacement fields).  Fields are (N, ndim, dims), fp32, contiguous; `dims` is
 * the spatial sizes in memory order, every one at least 2; channel c is the component along the axis dims[ndim - 1 - c] (channel
 * 0 runs along the last axis: the convention of the sampling grids).  D_j is the stencil of calculate_image_diff along axis j.
 * `mode`:  0                                        displacement: J_ij = delta_ij + D_j f_i
 *          ADVCHAIN_JACOBIAN_POSITIONS              the field is a sampling grid q in normalised [-1, 1] coordinates,
 *                                                   align_corners=True: J_ij = ((S_i - 1) / 2) D_j q_i, in voxel units (the
 *                                                   identity grid gives J = I)
 *          ADVCHAIN_JACOBIAN_POSITIONS | _CLAMP     q clamped to [-1, 1] as it is loaded -- what grid_sample(clamp_grid=True)
 *                                                   samples; the gradient passes where -1 <= q <= 1 (torch.clamp)
 * (the clamp without positions is refused.)  The file is compiled without contraction; the map and the statistics evaluate the
 * determinant with one device function, so the statistics are those of the map bit for bit.                               */
#define ADVCHAIN_JACOBIAN_POSITIONS 1
#define ADVCHAIN_JACOBIAN_CLAMP 2
/* in (N,C,S0,S1,S2) -> dx (along S2), dy (along S1), dz (along S0): 4 B read + 12 B written per element.                    */
int advchain_image_diff3d_fwd(const float* in, float* dx, float* dy, float* dz, int64_t N, int64_t C, const int64_t* dims,
                              void* stream);
/* its adjoint in gather form: grad_in = Dx^T grad_dx + Dy^T grad_dy + Dz^T grad_dz; any of the three may be NULL (zero), not all. */
int advchain_image_diff3d_bwd(const float* grad_dx, const float* grad_dy, const float* grad_dz, float* grad_in, int64_t N,
                              int64_t C, const int64_t* dims, void* stream);
/* det (N,1,dims) of field (N,ndim,dims), ndim 2 or 3.  ndim == 2 with mode 0 IS advchain_jacobian_det2d_fwd.                */
int advchain_jacobian_det_fwd(const float* field, float* det, int64_t N, int ndim, const int64_t* dims, int mode, void* stream);
/* grad f_i = s_i sum_j D_j^T (grad_det cof_ij), cofactors recomputed from `field` at the neighbours (gather form, no atomics:
 * two calls give the same bits).  `workspace`: advchain_jacobian_det_workspace floats, or NULL when that is 0 -- it is 0 for
 * every shape today (nothing is staged).  ndim == 2 with mode 0 IS advchain_jacobian_det2d_bwd.                             */
int advchain_jacobian_det_bwd(const float* grad_det, const float* field, float* grad_field, float* workspace, int64_t N,
                              int ndim, const int64_t* dims, int mode, void* stream);
int64_t advchain_jacobian_det_workspace(int64_t N, int ndim, const int64_t* dims); /* floats; host-only query */
/* One pass over the field, no determinant map.  Per batch entry n: neg[n] = #(det < 0), nonpos[n] = #(!(det > 0)) -- exact zeros
 * and NaN count, so a broken field cannot look clean; min[n], max[n] over the determinants that are numbers (NaN ignored; +inf
 * and -inf when there is none).  Every wave writes one partial into `workspace` (advchain_jacobian_stats_workspace floats,
 * 16-byte aligned; host-only query, -1 for bad sizes; no clearing needed) and one workgroup per entry folds them: integer sums
 * and min / max, no atomics -- bit-reproducible, and every output is written by a kernel of this call (no memset node under
 * capture).                                                                                                                 */
int64_t advchain_jacobian_stats_workspace(int64_t N, int ndim, const int64_t* dims); /* floats */
int advchain_jacobian_stats(const float* field, int64_t* neg, int64_t* nonpos, float* min, float* max, float* workspace,
                            int64_t N, int ndim, const int64_t* dims, int mode, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVCHAIN_HIP_H_ */
