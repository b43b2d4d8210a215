/* keymorph_hip.h -- C ABI of libkeymorph_hip.so (MI355X / gfx950 only).
 *
 * The reference (alanqrwang/keymorph @ 2.0.1) is pure Python on ATen: it has no
 * FFI of its own, so the drop-in boundary is the Python call surface of
 * keymorph/*  and THIS header is the native layer directly
 * underneath it -- one entry point per ATen call site of the hot path, each citing
 * the reference line(s) it replaces.  INTEGRATION.md shows the ctypes binding a
 * reference maintainer would add.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (hipMalloc / torch.cuda storage), fp32
 *     unless noted, densely packed in the stated layout;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - no allocation, no synchronisation, no ownership transfer inside; scratch
 *     is caller-provided (`ws`) and its size comes from the matching *_ws_bytes();
 *   - return value: 0 on success, otherwise the hipError_t of the failed launch
 *     or a negative KMH_E* code for bad arguments.
 */
#ifndef KEYMORPH_HIP_H
#define KEYMORPH_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define KMH_EINVAL (-22)
#define KMH_ABI_VERSION 1
int kmh_abi_version(void);

/* ---- a11: align_img = F.grid_sample(bilinear|nearest, border, align_corners=False)
 *      keymorph/utils.py:14-21.  x (N,C,D,H,W); grid (N,Do,Ho,Wo,3) xyz; out (N,C,Do,Ho,Wo).
 *      mode: 0 bilinear, 1 nearest. */
int kmh_grid_sample3d_fwd(const float* x, const float* grid, float* out, int N, int C, int D, int H,
                          int W, int Do, int Ho, int Wo, int mode, void* stream);
/* d(out)/d(grid) contracted with gout (N,C,Do,Ho,Wo) -> dgrid (N,Do,Ho,Wo,3) (bilinear). */
int kmh_grid_sample3d_bwd_grid(const float* x, const float* grid, const float* gout, float* dgrid,
                               int N, int C, int D, int H, int W, int Do, int Ho, int Wo, void* stream);
/* d(out)/d(x) contracted with gout -> dx (N,C,D,H,W), dx must be zero-filled by the caller. */
int kmh_grid_sample3d_bwd_input(const float* grid, const float* gout, float* dx, int N, int C, int D,
                                int H, int W, int Do, int Ho, int Wo, void* stream);

/* ---- a12: MSELoss, keymorph/loss_ops.py:9-13.  out[0] = mean((a-b)^2); ws >= kmh_reduce_ws_bytes(). */
size_t kmh_reduce_ws_bytes(void);
int kmh_mse_fwd(const float* a, const float* b, long long n, float* out, void* ws, void* stream);
/* da = gscale[0] * 2 (a-b)/n  (db = -da) */
int kmh_mse_bwd(const float* a, const float* b, const float* gscale, long long n, float* da, void* stream);
/* fused warp + MSE against `fixed` (same shape as out): writes out and out_loss[0]. */
int kmh_warp_mse_fwd(const float* x, const float* grid, const float* fixed, float* out, float* out_loss,
                     int N, int C, int D, int H, int W, int Do, int Ho, int Wo, void* ws, void* stream);
/* the same pass also writes dgrid = d(out_loss)/d(grid) (the MSE cotangent 2 (out - fixed) / count is known inside the
 * warp): align_img + MSELoss + autograd of both in ONE launch, 36 B per voxel instead of 68 in three; out may be NULL.
 * -22 when the shape needs the generic sampler (then use the separate entry points). */
int kmh_warp_mse_fwd_grad(const float* x, const float* grid, const float* fixed, float* out, float* out_loss,
                          float* dgrid, int N, int C, int D, int H, int W, int Do, int Ho, int Wo, void* ws,
                          void* stream);
/* a (n floats, n % 4 == 0) *= g[0], skipped on the device when g[0] == 1 (loss.backward() with the default cotangent) */
int kmh_scale_unless_one(float* a, long long n, const float* g, void* stream);

/* ---- a13: DiceLoss sums, keymorph/loss_ops.py:43-57.  pred/target (R, V) rows = n*c;
 *      sums (R,3) = {sum t*p, sum p*p, sum t*t}. */
int kmh_dice_sums(const float* pred, const float* target, int R, long long V, float* sums, void* ws,
                  void* stream);
/* out[r,i] = ca[r]*t[r,i] + cb[r]*p[r,i] (Dice backward wrt pred) */
int kmh_rows_axpby(const float* t, const float* p, const float* ca, const float* cb, int R, long long V,
                   float* out, void* stream);
/* ---- a11 + a13 fused (scripts/train.py:146-164 with the Dice loss): align_img (keymorph/utils.py:14-21) followed by
 *      the Dice sums (keymorph/loss_ops.py:28-52) WITHOUT storing the warped segmentation.
 *      sums[(n*C + c)*3 + {0,1,2}] = {sum t p, sum p^2, sum t^2}, p = grid_sample(x, grid)[n,c], t = fixed[n,c].
 *      -22 when the lane-contiguous sampler does not apply (W < 2, plane >= 2^31 voxels, C > 128). */
/* 1 when the fused warp + Dice entry points below serve these sizes (they return -22 otherwise): W >= 2, < 2^30 voxels per
 * channel plane, C <= 128, N * C <= 65536, the lane-contiguous sampler not switched off (KMH_SAMPLER_OLD).  The host asks
 * BEFORE building an autograd node and otherwise composes keymorph/utils.py:14-21 with keymorph/loss_ops.py:16-63 unfused. */
int kmh_warp_dice_ok(int N, int C, int D, int H, int W);
int kmh_warp_dice_sums(const float* x, const float* grid, const float* fixed, float* sums, int N, int C, int D, int H,
                       int W, int Do, int Ho, int Wo, const unsigned char* lab_x, const unsigned char* lab_fixed,
                       const int* gate, void* ws, void* stream);
/* its backward (autograd of keymorph/loss_ops.py:16-63 through keymorph/utils.py:14-21, one pass):
 *      dgrid[n,v,:] = sum_c (ca[n*C+c] t + cb[n*C+c] p) * d p / d grid, with ca = -2 g / den, cb = 2 g num / den^2. */
int kmh_warp_dice_bwd_grid(const float* x, const float* grid, const float* fixed, const float* ca, const float* cb,
                           float* dgrid, int N, int C, int D, int H, int W, int Do, int Ho, int Wo,
                           const unsigned char* lab_x, const unsigned char* lab_fixed, const int* gate, void* stream);
/*      lab_x (N, D*H*W) / lab_fixed (N, Do*Ho*Wo) / gate: all NULL, or the label maps and the device flag written by
 *      kmh_onehot_to_labels: one-hot segmentations (what keymorph/utils.py:200-240 + nearest-sampled augmentation produce,
 *      scripts/train.py:54-98) are then read as ONE byte per voxel (8 corner labels gathered once instead of 8 corner
 *      values per channel), bit-identical results; gate[0] == 0 (a soft segmentation) -> the float tensors are read. */
int kmh_onehot_to_labels(const float* x, int N, int C, long long V, unsigned char* lab, int* ok, void* stream);
/* hard Dice: onehot(argmax_c pred) over (N,C,V) -> out (N,C,V); first max wins like torch.argmax */
int kmh_argmax_onehot(const float* pred, int N, int C, long long V, float* out, void* stream);
/* keymorph/loss_ops.py:161-247 (_jacobian_determinant, jdstd, jdlessthan0): central differences with zero padding
 * + identity, cropped by 2 voxels; component c of voxel v at disp[c*cstride + v*vstride].  jd (D-4,H-4,W-4) or
 * NULL; stats[4] (double) = {mean, population std, #(det <= 0), #voxels}; ws = kmh_reduce_ws_bytes(). */
int kmh_jacobian_det(const float* disp, long long cstride, long long vstride, int D, int H, int W, float* jd,
                     double* stats, void* ws, void* stream);

/* ---- label-map encodings in front of the Dice branch: keymorph/utils.py:200-240 (one_hot,
 * one_hot_subsampled_pair; callers scripts/train.py:54-61) ---- */
/* flags: nflags + 1 ints zeroed by the caller; flags[l] = 1 iff label l occurs among the n int64 values of seg,
 * flags[nflags] = 1 iff a label lies outside [0, nflags) (replaces np.unique on the host). */
int kmh_label_presence(const long long* seg, long long n, int nflags, int* flags, void* stream);
/* out[n,c,v] = (seg[n,v] == labels[c]), C <= 256; float32 out (out_i64 = 0) or int64 out like F.one_hot (1). */
int kmh_one_hot_select(const long long* seg, int N, long long V, const long long* labels, int C, void* out,
                       int out_i64, void* stream);

/* ---- evaluation metrics: keymorph/loss_ops.py:66-158 (fast_dice, dice, hausdorff_distance) ---- */
/* a, b: channel 0 of N samples (sample n at + n * sstride elements, each (D,H,W) contiguous); dtype 0 f32, 1 f64, 2 f16,
 * 3 bf16, 4 one byte, 5 int16, 6 int32, 7 int64, a voxel is set iff its value != 0.  out_sq[n] = squared Hausdorff distance
 * of the two 6-connected surfaces with spacing (sz, sy, sx) along (D, H, W): +inf if one surface is empty, NaN if both are.
 * ws: kmh_hausdorff3d_ws_bytes(D, H, W) bytes (per sample; samples run one after the other). */
size_t kmh_hausdorff3d_ws_bytes(int D, int H, int W);
int kmh_hausdorff3d(const void* a, const void* b, int dtype_a, int dtype_b, long long sstride_a, long long sstride_b, int N,
                    int D, int H, int W, double sz, double sy, double sx, void* ws, double* out_sq, void* stream);
/* the squared distance map of one mask's surface (same passes; tests): out (D,H,W) fp64, +inf if the surface is empty */
size_t kmh_edt3d_sq_ws_bytes(int D, int H, int W);
int kmh_edt3d_sq(const void* a, int dtype, int D, int H, int W, double sz, double sy, double sx, void* ws, double* out,
                 void* stream);
/* counts (3 * nlab uint64, zeroed by the caller) = {|x = l|, |y = l|, |x = l and y = l|}; C > 0: labels = channel argmax of
 * (N, C, V) maps of dtype 0 f32 / 1 f64, nlab = C <= 4096; C == 0: labels = (byte != 0) of N * V bytes, nlab = 2. */
int kmh_label_counts(const void* x, const void* y, int dtype, int N, int C, long long V, unsigned long long* counts,
                     void* stream);

/* ---- LC2 / ImageLC2 similarity: keymorph/loss_ops.py:250-391 (LC2.forward/run :262-302, ImageLC2.forward/run :335-391) ---- */
/* us, mr: (N, S, S, S) contiguous, tiled into P^3 patches without overlap (nP = S / P per axis, the remainder dropped; patch
 * ((n nP + pz) nP + py) nP + px, B = N nP^3; LC2 is P = S).  radii: HOST array of R <= 8 radii, each with P - (2r + 1) even
 * and >= 2, r <= 511.  out: B floats = per patch the mean over the radii of clamp((var - dist) / max(var, beta), 0, 1), or one float
 * (reduce_mean != 0) = their mean.  ws: kmh_lc2_ws_bytes(B, R) bytes, written here and read by kmh_lc2_bwd. */
size_t kmh_lc2_ws_bytes(int num_patches, int num_radii);
int kmh_lc2_fwd(const float* us, const float* mr, int N, int S, int P, const int* radii, int R, double alpha, double beta,
                int reduce_mean, void* ws, float* out, void* stream);
/* the reference's autograd of the same: gout = B floats (or one with reduce_mean); dus, dmr (N, S, S, S), every voxel written
 * (zero outside the crops and their 1-voxel halos); either may be NULL. */
int kmh_lc2_bwd(const float* us, const float* mr, const float* gout, int N, int S, int P, const int* radii, int R,
                int reduce_mean, const void* ws, float* dus, float* dmr, void* stream);

/* ---- mutual information through a Parzen-window joint histogram (csrc/mi.hip states the definition) ---- */
/* a, b: (N, V) float32 contiguous, 8 <= bins <= 64.  kmh_mi_hist: per-sample ranges (has_range_x != 0: the caller's (lo_x, hi_x)
 * instead of the image's minimum and maximum) -> rng (N, 4) = (lo_a, s_a, lo_b, s_b), and the fixed-point joint table in ws
 * (kmh_mi_ws_bytes(N, bins) bytes).  kmh_mi_final: the table -> mi (N floats) and G (N, bins, bins) = ln(p / (pa pb)) where
 * p > 0, else 0.  kmh_mi_bwd: da = gout[n] dMI_n / da, db likewise, (N, V) float32, either may be NULL. */
size_t kmh_mi_ws_bytes(int N, int bins);
int kmh_mi_hist(const float* a, const float* b, int N, long long V, int bins, int has_range_a, float lo_a, float hi_a,
                int has_range_b, float lo_b, float hi_b, void* ws, float* rng, void* stream);
int kmh_mi_final(const void* ws, const float* rng, int N, long long V, int bins, float* mi, float* G, void* stream);
int kmh_mi_bwd(const float* a, const float* b, const float* rng, const float* G, const float* gout, int N, long long V,
               int bins, float* da, float* db, void* stream);
/* kmh_mi_hist's ranges alone: rng (N, 4) out, ws 16 N bytes. */
int kmh_mi_range(const float* a, const float* b, int N, long long V, int bins, int has_range_a, float lo_a, float hi_a,
                 int has_range_b, float lo_b, float hi_b, void* ws, float* rng, void* stream);
/* kmh_mi_hist with the ranges given on the device: rng (N, 4) in, as kmh_mi_range wrote it; kmh_mi_final and kmh_mi_bwd follow. */
int kmh_mi_hist_ranges(const float* a, const float* b, const float* rng, int N, long long V, int bins, void* ws, void* stream);
/* The same over the COUNTED voxels only: mask (N, V) bytes, non-zero = counted, NULL = every voxel.  cnt: N 64-bit integers on
 * the device, the number of counted voxels per sample, written by the histogram pass and read by the other two (the host never
 * reads it): p = h / cnt[n], gradients scaled by 1 / cnt[n], 0 at a voxel that is not counted; cnt[n] = 0: MI = 0, G = 0. */
int kmh_mi_hist_masked(const float* a, const float* b, const unsigned char* mask, const float* rng, int N, long long V, int bins,
                       void* ws, long long* cnt, void* stream);
int kmh_mi_final_masked(const void* ws, const float* rng, const long long* cnt, int N, int bins, float* mi, float* G,
                        void* stream);
int kmh_mi_bwd_masked(const float* a, const float* b, const unsigned char* mask, const float* rng, const float* G,
                      const float* gout, const long long* cnt, int N, long long V, int bins, float* da, float* db, void* stream);

/* ---- mutual information of a fixed volume and a moving volume warped by a matrix, fused (csrc/warp_mi.hip) ---- */
/* By definition MI(grid_sample3d(moving, affine_grid(mat)), fixed) with the ranges rng = kmh_mi_range(moving, fixed): moving,
 * fixed (N, D, H, W) float32, mat (N, 3, 4), 8 <= bins <= 64, W >= 2, fewer than 2^30 voxels per sample (else -22).
 * kmh_warp_mi_hist leaves the joint table in ws (kmh_warp_mi_ws_bytes bytes) in kmh_mi_hist's layout: kmh_mi_final(ws, rng, N,
 * D H W, bins, mi, G) follows.  kmh_warp_mi_bwd: dmat (N, 3, 4) = gout[n] dMI_n / dmat, deterministic, a batch equals its samples. */
size_t kmh_warp_mi_ws_bytes(int N, int bins, int D, int H, int W);
int kmh_warp_mi_hist(const float* moving, const float* fixed, const float* mat, const float* rng, int N, int D, int H, int W,
                     int bins, void* ws, void* stream);
int kmh_warp_mi_bwd(const float* moving, const float* fixed, const float* mat, const float* rng, const float* G,
                    const float* gout, int N, int D, int H, int W, int bins, void* ws, float* dmat, void* stream);
/* The same over the counted voxels only.  Fixed-lattice voxel v with sampling coordinate g(v) is counted iff fixed_mask[v] != 0,
 * moving_mask != 0 at the nearest sampler's voxel for g(v), and (inside != 0) every |g(v)_k| <= 1; masks (N, D, H, W) bytes, either
 * may be NULL.  cnt as in kmh_mi_hist_masked; kmh_mi_final_masked follows the histogram pass.  Same workspace. */
int kmh_warp_mi_hist_masked(const float* moving, const float* fixed, const unsigned char* fixed_mask,
                            const unsigned char* moving_mask, const float* mat, const float* rng, int N, int D, int H, int W,
                            int bins, int inside, void* ws, long long* cnt, void* stream);
int kmh_warp_mi_bwd_masked(const float* moving, const float* fixed, const unsigned char* fixed_mask,
                           const unsigned char* moving_mask, const float* mat, const float* rng, const float* G,
                           const float* gout, const long long* cnt, int N, int D, int H, int W, int bins, int inside, void* ws,
                           float* dmat, void* stream);

/* ---- a9: AffineTransform.get_flow_field, keymorph/transformations.py:37-79 and
 *      uniform_norm_grid keymorph/utils.py:387-398.  mat (N,3,4) = inverse_transform_matrix[:, :3, :]
 *      acting on ij coords; out (N,D,H,W,3) already flipped to xyz. */
int kmh_affine_grid_fwd(const float* mat, float* out, int N, int D, int H, int W, void* stream);
int kmh_affine_grid_bwd(const float* dgrid, float* dmat, int N, int D, int H, int W, void* ws, void* stream);

/* ---- a8: TPS.get_flow_field / transform_points, keymorph/keypoint_aligners.py:365-433.
 *      theta (N,T+4,3) rows [w_0..w_{T-1}, a_0, a_z, a_y, a_x]; ctrl (N,T,3) ij; out (N,D,H,W,3) xyz. */
int kmh_tps_grid_fwd(const float* theta, const float* ctrl, float* out, int N, int T, int D, int H, int W,
                     void* stream);
size_t kmh_tps_grid_bwd_ws_bytes(int N, int T, int D, int H, int W);
int kmh_tps_grid_bwd(const float* dgrid, const float* theta, const float* ctrl, float* dtheta,
                     float* dctrl, int N, int T, int D, int H, int W, void* ws, void* stream);
/* same spline evaluated at explicit points (N,P,3) ij -> out (N,P,3) ij (a10: points_a). */
int kmh_tps_points_fwd(const float* theta, const float* ctrl, const float* pts, float* out, int N, int T,
                       int P, void* stream);
size_t kmh_tps_points_bwd_ws_bytes(int N, int T, int P);
int kmh_tps_points_bwd(const float* dout, const float* theta, const float* ctrl, const float* pts,
                       float* dtheta, float* dctrl, float* dpts, int N, int T, int P, void* ws,
                       void* stream);

/* ---- a7: TPS.fit, keymorph/keypoint_aligners.py:276-363.  Assembles A = [[U+lambda I, P],[P^T,0]]
 *      in fp32 exactly as the reference, factorises in fp64 (partial-pivot LU, one workgroup per
 *      sample) and solves 3 right-hand sides.  ctrl,tgt (N,T,3); lmbda (N); w (N,T) or NULL;
 *      theta (N,T+4,3).  ws keeps the LU factors + pivots for the backward. */
size_t kmh_tps_fit_ws_bytes(int N, int T);
int kmh_tps_fit_fwd(const float* ctrl, const float* tgt, const float* lmbda, const float* w, float* theta,
                    int N, int T, void* ws, void* stream);
/* Large systems are factorised by a cluster of workgroups per system that hand panels over through global counters; a
 * cluster that could not get all its workgroups resident gives up (bounded waits) and the SAME call redoes that system on
 * the one-workgroup kernel (device-side retry pass, no host round trip).  Test hook: the next `count` clustered calls mark
 * every system as "gave up" so that the retry pass does all the work; returns the previous count. */
int kmh_tps_fit_force_retry(int count);
/* backward: given dtheta -> dctrl, dtgt (uses the factors in ws written by the forward) and, when the fit was
 * weighted and dw != NULL, dw (N,T) = d/dw of the lmbda / (w + 1e-6) diagonal. */
int kmh_tps_fit_bwd(const float* dtheta, const float* theta, const float* ctrl, const float* lmbda, const float* w,
                    float* dctrl, float* dtgt, float* dw, int N, int T, void* ws, void* stream);

/* ---- a5/a6: closed-form affine (keymorph/keypoint_aligners.py:76-114) and rigid/Kabsch
 *      (:151-213) fits.  x,y (N,K,3); w (N,K) or NULL; M (N,3,4). */
int kmh_affine_fit_fwd(const float* x, const float* y, const float* w, float* M, int N, int K, void* stream);
/* backwards: dw (N,K) or NULL = gradient w.r.t. the keypoint weights (needs w != NULL). */
int kmh_affine_fit_bwd(const float* dM, const float* x, const float* y, const float* w, const float* M,
                       float* dx, float* dy, float* dw, int N, int K, void* stream);
int kmh_rigid_fit_fwd(const float* x, const float* y, const float* w, float* M, int N, int K, void* stream);
int kmh_rigid_fit_bwd(const float* dM, const float* x, const float* y, const float* w, float* dx, float* dy,
                      float* dw, int N, int K, void* stream);
/* 4x4 homogeneous inverse of [M;0 0 0 1] (keymorph/transformations.py:23-35) and its backward. */
int kmh_affine_inverse_fwd(const float* M, float* Minv, int N, void* stream);
int kmh_affine_inverse_bwd(const float* dMinv, const float* Minv, float* dM, int N, void* stream);
/* points (N,P,3) -> M[:, :3, :] @ [p;1] (keymorph/transformations.py:81-114) */
int kmh_affine_points_fwd(const float* M, const float* pts, float* out, int N, int P, void* stream);
/* keymorph/augmentation.py:85-158 AffineDeformation3d.build_affine_matrix: scale (B,3), offset (B,3), theta (B,3),
 * shear (B,6) -> out (B,4,4) = Mz Ms Mt (R3 R2 R1) */
int kmh_affine_build_matrix(const float* scale, const float* offset, const float* theta, const float* shear,
                            float* out, int B, void* stream);
int kmh_affine_points_bwd(const float* dout, const float* M, const float* pts, float* dM, float* dpts,
                          int N, int P, void* stream);

/* ---- a4: CenterOfMass3d, keymorph/layers.py:78-134.  feat (N,K,D,H,W) -> pts (N,K,3) (z,y,x)
 *      in [-1,1]; sums (N,K,4) = {m, mz, my, mx} kept for the backward. */
int kmh_com3d_fwd(const float* feat, float* pts, float* sums, int N, int K, int D, int H, int W, void* ws,
                  void* stream);
int kmh_com3d_bwd(const float* dpts, const float* feat, const float* sums, float* dfeat, int N, int K,
                  int D, int H, int W, void* stream);


/* ==== a2/a3: backbone operators.  Activations are NDHWC (N, D, H, W, C) fp32 internally. ==== */

/* conv3d k=3 p=1 s=1 (keymorph/unet3d/buildingblocks.py:46-58, keymorph/layers.py:173-175) on the
 * fp32 matrix cores.  pack: torch (Cout,Cin,3,3,3) -> [27][Cin][Cout] (transposed=0, forward) or the
 * tap-mirrored [27][Cout][Cin] (transposed=1) that turns the SAME kernel into the data gradient.
 * fwd: y = act_out( conv( act_in(x*scale[n,c]+shift[n,c]) * [mask > 0] ) + bias ); scale/shift/mask/bias may be
 * NULL.  `mask` (same shape as x) fuses the ReLU backward into the data-gradient pass (x = dy, mask = y). */
int kmh_conv3d_pack_weight(const float* w, float* packed, int Cout, int Cin, int transposed, void* stream);
int kmh_conv3d_fwd(const float* x, const float* scale, const float* shift, const float* mask,
                   const float* packed_w, const float* bias, float* y, int N, int D, int H, int W, int Cin,
                   int Cout, int relu_in, int relu_out, void* stream);
/* Split-operand variant of the same convolution (csrc/conv_bf.hip; fused decoder operator csrc/conv_up2.hip, weight gradient
 * csrc/conv_wgrad.hip): fp32 operands are split into 16-bit pieces and
 * multiplied on the 16-bit matrix cores with fp32 accumulation.  terms = 2 ("f16x3", the host default): operands
 * range-scaled by powers of two (ascale / wscale = {S, 1/S} device pairs, see kmh_absmax_scale) and split into fp16
 * hi + lo, 3 MFMAs per product block; terms = 3 ("bf16x6"): bf16 hi + mid + lo, 6 MFMAs, no scales.  Both are
 * fp32-class (5e-7 vs fp64).  Same semantics / arguments as kmh_conv3d_pack_weight + kmh_conv3d_fwd, with its own
 * packed layout. */
size_t kmh_conv3d_pack_bf_bytes(int Cout, int Cin, int transposed, int terms);
int kmh_conv3d_pack_weight_bf(const float* w, void* packed, int Cout, int Cin, int transposed, int terms,
                              const float* wscale, void* stream);
/* stats_out (N,Cout,2) doubles | NULL: per-channel (sum y, sum y^2) of the OUTPUT from the epilogue -- what
 * kmh_channel_stats(y) returns, i.e. the next GroupNorm's statistics without another pass over y; stats_ws holds the
 * per-brick partials (kmh_conv3d_fwd_bf_stats_ws_bytes). */
size_t kmh_conv3d_fwd_bf_stats_ws_bytes(int N, int D, int H, int W, int Cout, int rows_per_wave);
int kmh_conv3d_fwd_bf(const float* x, const float* scale, const float* shift, const float* mask, const void* packed,
                      const float* bias, float* y, int N, int D, int H, int W, int Cin, int Cout, int relu_in,
                      int relu_out, int terms, int rows_per_wave, const float* ascale, const float* wscale,
                      void* stats_ws, double* stats_out, int in_blocked, const float* addend, void* stream);
/* Kernel selection of kmh_conv3d_fwd_bf (the reference has one conv3d: keymorph/unet3d/buildingblocks.py:46-58; this
 * only chooses between two implementations with bit-identical results).  mode 0: conv3_fwd_bf_kernel always; 1: the
 * LDS-DMA kernel conv3_fwd_g_kernel for launches of >= 512 bricks (default; KEYMORPH_FWD_G sets the initial value);
 * 2: conv3_fwd_g_kernel whenever its preconditions hold (parity tests on small / ragged volumes).  Returns the
 * previous mode, -22 for a bad argument. */
int kmh_conv3d_fwd_bf_set_dispatch(int mode);
/* use_amp (keymorph/model.py:176-191 autocasts the keypoint extractor to fp16) is PER CALL: every launching entry point below
 * that takes `terms` -- kmh_conv3d_fwd_bf, kmh_conv3d_fwd_bf_pool, kmh_conv3d_wgrad_bf, kmh_conv3d_up2_fwd, kmh_conv3d_up2_dgrad,
 * kmh_up2_wgrad_gemm, kmh_up2_wgrad_fold, kmh_headcom_fwd_bf, kmh_headcom_bwd_bf -- accepts terms == 1 = "the fp16 kernels of
 * terms == 2 with only the hi x hi product": fp16 inputs (11 significant bits), fp32 accumulation, one MFMA per product block
 * instead of three.  Packing, scales, layouts, workspaces and the *_ok / *_bytes queries are those of terms == 2 (pass 2
 * there).  There is no process-wide switch: the caller that ran a forward with terms == 1 passes 1 to its backward calls. */
/* in_blocked of kmh_conv3d_fwd_bf: 0 = x is (N,D,H,W,Cin); 1 = channel-blocked (N,Cin/8,D,H,W,8) fp32; 2 = PRE-SPLIT
 * channel-blocked: (N, Cin/8, D*H*W + 1) records of 32 bytes, the 8 fp16 "hi" then the 8 fp16 "lo" terms of fmaf(value, S, 0)
 * with S = ascale[0], record D*H*W of every plane zero -- what kmh_maxpool3d_bwd_split writes; the kernel then copies
 * fragments (LDS-DMA) instead of converting them, with bit-identical results (conv3_fwd_s_kernel<1,true,true>).  Mode 2 serves
 * gradient operands (no scale / shift / mask / relu_in / addend) of the z-paired tile (Cout <= 16): kmh_conv3d_fwd_bf_split_ok
 * returns 1 for the shapes it takes, kmh_conv3d_fwd_bf returns -22 for the others.  Replaces the data gradient of
 * keymorph/unet3d/buildingblocks.py:46-58 (autograd of conv3d) behind a pooling layer (:321-380). */
int kmh_conv3d_fwd_bf_split_ok(int N, int D, int H, int W, int Cin, int Cout, int terms);
/* The same operand WITHOUT the scatter ("pooled + winners", layout kind 3 of the backbone's gradient hand-off): xp (N, D/2, H/2,
 * W/2, Cin) fp32 = the pooled gradient, winners (same shape, bytes) = the window indices 0..7 = (dz, dy, dx) of
 * kmh_conv3d_fwd_bf_pool / kmh_maxpool3d_fwd; the kernel builds in its own staging the fragment images the pre-split records
 * would give (the dense tensor, 7/8 zeros, is never written or read).  y and stats_out are bit-identical to in_blocked == 2.
 * kmh_conv3d_fwd_bf_sparse_ok: 1 for the shapes served (those of kmh_conv3d_fwd_bf_split_ok with even D, H, W, terms == 2 -- not
 * use_amp's terms == 1), whatever the dispatch mode; -22 from kmh_conv3d_fwd_bf_sparse elsewhere.  Replaces
 * MaxPool3d's backward (keymorph/unet3d/buildingblocks.py:321-380) followed by conv3d's data gradient (:46-58). */
int kmh_conv3d_fwd_bf_sparse_ok(int N, int D, int H, int W, int Cin, int Cout, int terms);
int kmh_conv3d_fwd_bf_sparse(const float* xp, const unsigned char* winners, const void* packed, const float* bias, float* y,
                             int N, int D, int H, int W, int Cin, int Cout, int relu_out, int terms, const float* ascale,
                             const float* wscale, void* stats_ws, double* stats_out, void* stream);
/* the kernel kmh_conv3d_fwd_bf would launch for this call now: 0 conv3_fwd_bf_kernel, 1 / 2 conv3_fwd_g_kernel with a
 * 32- / 64-wide output-channel tile, 3 its z-paired variant (Cout <= 16) */
int kmh_conv3d_fwd_bf_variant(int N, int D, int H, int W, int Cin, int Cout, int terms, int has_mask, int has_addend);
/* GroupNorm -> Conv3d -> ReLU -> MaxPool3d(2) in one launch (keymorph/unet3d/buildingblocks.py:46-78 followed by the next
 * Encoder's `self.pooling`, :321-380), for a block whose output feeds only that pooling: yp (N, D/2, H/2, W/2, Cout) the
 * pooled output, arg (same shape, bytes) the winners' window indices in kmh_maxpool3d_fwd's format (ATen's first-max
 * rule), stats_out (N, Cout, 2) the pooled tensor's (sum, sum^2); the full-resolution output is not written.
 * kmh_conv3d_fwd_bf_pool_ok: 1 when the shape is served (16 < Cout <= 32, Cin % 8 == 0, terms == 2, LDS-DMA kernel). */
int kmh_conv3d_fwd_bf_pool_ok(int N, int D, int H, int W, int Cin, int Cout, int terms);
int kmh_conv3d_fwd_bf_pool(const float* x, const float* scale, const float* shift, const void* packed, float* yp,
                           unsigned char* arg, int N, int D, int H, int W, int Cin, int Cout, int relu_in, int terms,
                           const float* ascale, const float* wscale, void* stats_ws, double* stats_out, int in_blocked,
                           void* stream);
/* addend (like y) | NULL: added to the result before the activation and the statistics (Cout > 16).
 * Decoder's first convolution without the upsampled tensor: the 27 taps over a nearest-x2 upsampled channel fall on
 * 2 x 2 x 2 low-resolution voxels per output parity, so kmh_conv3d_up2_fwd computes the upsampled channels'
 * contribution from the LOW-resolution tensor with 8 (pre-summed) taps instead of 27, and kmh_conv3d_fwd_bf over the
 * skip channels adds it (keymorph/unet3d/buildingblocks.py:471-475 nearest interpolate + cat, then :46-78). */
size_t kmh_conv3d_up2_pack_bytes(int Cout, int Cl, int terms);
int kmh_conv3d_up2_pack_weight(const float* w, void* packed, int Cout, int Ctot, int cofs, int Cl, int terms,
                               const float* wscale, void* stream);
/* data gradient of the same operator: ds (N,Dl,Hl,Wl,Cl) = per low voxel, the sum over its 8 children of the gradient
 * with respect to the upsampled tensor (what interpolate's backward would sum), from dz (N,2Dl,2Hl,2Wl,Cout): 64
 * pre-summed taps at low resolution instead of 8 x 27 at high resolution */
size_t kmh_conv3d_up2_dgrad_pack_bytes(int Cout, int Cl, int terms);
int kmh_conv3d_up2_dgrad_pack_weight(const float* w, void* packed, int Cout, int Ctot, int cofs, int Cl, int terms,
                                     const float* wscale, void* stream);
/* stats_out (N,Cl,2) doubles | NULL: per-channel (sum ds, sum ds^2) from the epilogue (what GroupNorm's backward of the
 * decoder block needs from this gradient: no separate pass over ds); stats_ws: ..._stats_ws_bytes (may be NULL with it) */
size_t kmh_conv3d_up2_dgrad_stats_ws_bytes(int N, int Dl, int Hl, int Wl, int Cl);
int kmh_conv3d_up2_dgrad(const float* dz, const void* packed, float* ds, int N, int Dl, int Hl, int Wl, int Cl, int Cout,
                         int terms, const float* dscale, const float* wscale, void* stats_ws, double* stats_out,
                         int in_blocked /* dz channel-blocked (N, Cout/8, 2Dl, 2Hl, 2Wl, 8): whole lines per request */,
                         void* stream);
/* weight gradient of the same operator (csrc/norm.hip): G (N, Dl*Hl*Wl, 27, Cout) = 2x2x2 box sums of dz such that
 * dW[tap][ci][co] = sum_m x_low[m][ci] G[m][tap][co] -- one plain matrix product over the low-resolution voxels */
int kmh_up2_boxsum(const float* dz, float* G, int N, int Dl, int Hl, int Wl, int Cout, int in_blocked /* as above */,
                   void* stream);
/* C (N, Cl, J) = A^T B per sample over the V low-resolution voxels: A (N, V, Cl) the normalised low tensor, B (N, V, J)
 * the box sums with J = 27 Cout (split-operand MFMA; ascale / bscale = {S, 1/S} of A and B for terms == 2).
 * a_scale / a_shift (N, Cl) | both NULL: A is the RAW low tensor and GroupNorm's affine a_scale[n][c] A + a_shift[n][c]
 * (keymorph/unet3d/buildingblocks.py:46-78, "g" of "gcr") is applied while it is staged; ascale is then the range scale
 * of the normalised values */
size_t kmh_up2_wgrad_gemm_ws_bytes(int N, int V, int Cl, int J);
int kmh_up2_wgrad_gemm(const float* A, const float* B, float* C, int N, int V, int Cl, int J, int terms,
                       const float* ascale, const float* bscale, const float* a_scale, const float* a_shift, void* ws,
                       void* stream);
/* Round 5: the two calls above in ONE product, the box sums formed on the fly from dz (never stored): C (N, Cl, 27 Cout) for
 * xl (N, Dl, Hl, Wl, Cl) the RAW low tensor (a_scale / a_shift (N, Cl): GroupNorm's affine, or both NULL), dz (N, 2Dl, 2Hl,
 * 2Wl, Cout) or channel-blocked (dz_blocked != 0), ascale / dscale = {S, 1/S} range scales of the normalised low tensor and
 * of dz (the box sums are scaled by S / 8).  fp16 split only (terms == 2), Cl % 4 == 0, Cout % 8 == 0: kmh_up2_wgrad_fold_ok.
 * Replaces autograd's weight gradient of interpolate(nearest x2) + cat + conv3d for the upsampled channels
 * (keymorph/unet3d/buildingblocks.py:471-475, :46-78). */
int kmh_up2_wgrad_fold_ok(int Cl, int Cout, int terms);
size_t kmh_up2_wgrad_fold_ws_bytes(int N, int Dl, int Hl, int Wl, int Cl, int Cout);
int kmh_up2_wgrad_fold(const float* xl, const float* dz, float* C, int N, int Dl, int Hl, int Wl, int Cl, int Cout, int terms,
                       const float* ascale, const float* dscale, const float* a_scale, const float* a_shift, int dz_blocked,
                       void* ws, void* stream);
int kmh_conv3d_up2_fwd(const float* xl, const float* scale, const float* shift, int Ctot, int cofs, const void* packed,
                       float* y, int N, int Dl, int Hl, int Wl, int Cl, int Cout, int terms, const float* ascale,
                       const float* wscale, void* stream);
/* in_blocked != 0 (here) / dz_blocked != 0 (weight gradient) / out_blocked != 0 (kmh_gn_bwd_apply): that tensor is
 * stored channel-blocked, (N, C/8, D, H, W, 8) instead of (N, D, H, W, C): the 8 channels of one chunk of one voxel
 * are a 32-byte record and a chunk's voxels are contiguous, so the conv loader uses whole cache lines.  Internal
 * layout of gradients handed from one SingleConv to the one before it; C % 8 == 0, no ReLU mask operand, results
 * bit-identical to the (N, D, H, W, C) path. */
/* split-bf16 weight gradient (same semantics as kmh_conv3d_wgrad; terms = 2 | 3) */
size_t kmh_conv3d_wgrad_bf_ws_bytes(int N, int D, int H, int W, int Cin, int Cout, int terms);
int kmh_conv3d_wgrad_bf_blocked_ok(int N, int D, int H, int W, int Cin, int Cout, int terms); /* 1: accepts dz_blocked */
int kmh_conv3d_wgrad_bf(const float* x, const float* scale, const float* shift, const float* dz,
                        const float* dzmask, float* dw, int N, int D, int H, int W, int Cin, int Cout, int relu_in,
                        int accumulate, int terms, int append_ones, const float* xscale, const float* dscale, int dz_blocked, const float* w_fold, double* bhat,
                        void* ws, void* stream);
/* The same weight gradient from the POOLED gradient dzp (N, D/2, H/2, W/2, Cout) and its winner bytes (see
 * kmh_conv3d_fwd_bf_sparse): bit-identical to dz_blocked == 2 on the scattered records.  kmh_conv3d_wgrad_bf_sparse_ok: 1 where
 * served (the shapes of kmh_conv3d_wgrad_bf_blocked_ok with even D, H, W, terms == 2). */
int kmh_conv3d_wgrad_bf_sparse_ok(int N, int D, int H, int W, int Cin, int Cout, int terms);
int kmh_conv3d_wgrad_bf_sparse(const float* x, const float* scale, const float* shift, const float* dzp,
                               const unsigned char* winners, float* dw, int N, int D, int H, int W, int Cin, int Cout,
                               int relu_in, int accumulate, int terms, const float* xscale, const float* dscale,
                               const float* w_fold, double* bhat, void* ws, void* stream);
/* First U-Net convolution, forward (csrc/firstlayer.hip): x (N,D,H,W) raw 1-channel input, scale / shift (N)
 * GroupNorm coefficients of that channel (NULL: identity), w (Cout,1,3,3,3), Cout <= 16 ->
 * y (N,D,H,W,Cout) = relu(conv3(x * scale + shift)) in exact fp32 (keymorph/unet3d/buildingblocks.py:46-78 for
 * encoders[0].SingleConv1); stats_out (N,Cout,2) doubles | NULL = (sum y, sum y^2) as in kmh_conv3d_fwd_bf. */
size_t kmh_conv3d_first_layer_fwd_ws_bytes(int N, int D, int H, int W, int Cout);
int kmh_conv3d_first_layer_fwd(const float* x, const float* scale, const float* shift, const float* w, float* y, int N,
                               int D, int H, int W, int Cout, void* ws, double* stats_out, void* stream);
/* first U-Net layer (Cin = 1), backward of keymorph/unet3d/buildingblocks.py:46-78 for encoders[0] without the
 * 1-channel data gradient: rs (N,Cout,2,27) (doubles; rs_f64 = 1 in the fold) = correlations of dz with the RAW input (R) and with the indicator of the
 * volume (S), by a dedicated exact-fp32 kernel (Cout <= 16); then ... */
size_t kmh_conv3d_first_layer_wgrad_ws_bytes(int N, int D, int H, int W, int Cout);
/* c123 (N,Cout,3) | NULL (needs dzmask): the gradient entering the correlations is [dzmask > 0] (c1 dz + c2 dzmask + c3)
 * -- the NEXT layer's GroupNorm backward (what kmh_gn_bwd_apply would have written) applied while dz is staged */
int kmh_conv3d_first_layer_wgrad(const float* x, const float* dz, const float* dzmask, const float* c123, double* rs, int N,
                                 int D, int H, int W, int Cout, void* ws, void* stream);
/* ... fold the (x, 1) correlations of one sample into dw and GroupNorm's (A, B) sums */
int kmh_conv3d_first_layer_fold(const void* rs, int rs_f64, const float* w, const float* scale_n, const float* shift_n, int Cout,
                                float* dw, double* ab_n, int accumulate, void* stream);
/* dw (Cout,Cin,3,3,3) (+)= sum_v act_in(x*scale+shift)[v+tap] dz[v]*[dzmask[v] > 0]  (dzmask may be NULL) */
size_t kmh_conv3d_wgrad_ws_bytes(int N, int D, int H, int W, int Cin, int Cout);
int kmh_conv3d_wgrad(const float* x, const float* scale, const float* shift, const float* dz,
                     const float* dzmask, float* dw, int N, int D, int H, int W, int Cin, int Cout, int relu_in,
                     int accumulate, void* ws, void* stream);

/* per-(n,c) sums over V voxels of an (N,V,C) tensor: mode 0 -> (sum a, sum a^2), mode 1 -> (sum a, sum a*b);
 * out (N,C,2) doubles.  Feeds GroupNorm (buildingblocks.py:59-78) / InstanceNorm (layers.py:165). */
size_t kmh_channel_stats_ws_bytes(int N, int C);
int kmh_channel_stats(const float* a, const float* b, int mode, int N, long long V, int C, double* out, void* ws,
                      const int* only_if, void* stream);
/* stats -> scale = rstd*gamma, shift = beta - mean*rstd*gamma per (n,c); mean_rstd (N,G,2).
 * count = elements per channel (voxels).  gamma/beta NULL = instance norm without affine. */
int kmh_gn_fwd_coeffs(const double* stats, const float* gamma, const float* beta, int N, int C, int G, double count,
                      float eps, float* scale, float* shift, float* mean_rstd, float* ascale, void* stream);
/* Range scales for the fp16-split ("f16x3", terms = 2) convolutions: device float[2] = {S, 1/S}, S a power of two.
 * kmh_gn_fwd_coeffs(ascale != NULL) writes the scale of the NORMALISED tensor from the guaranteed bound
 * max|gamma| sqrt(elements per group) + max|beta|; kmh_absmax_scale measures max(max|x|, min_abs) of a tensor. */
int kmh_absmax_scale(const float* x, long long n, float min_abs, float* out2, void* stream);
/* ab (N,C,2) = (sum dxn, sum dxn*x) -> c123 (N,C,3) with dx = c1*dxn + c2*x + c3; dgamma/dbeta (C) += */
int kmh_gn_bwd_coeffs(const double* ab, const float* gamma, const float* mean_rstd, int N, int C, int G,
                      double count, float* c123, float* dgamma, float* dbeta, const int* only_if, void* stream);
/* GroupNorm backward coefficients from statistics that need no pass over the tensors (csrc/norm.hip): dstats (N,C,2)
 * with [.][0] = sum_v dxn (the epilogue statistics `stats_out` of the data-gradient launch), bhat (N,C) = sum_v dxn *
 * xhat from kmh_conv3d_wgrad_bf(w_fold = the layer's weights (Cout,Cin,27), bhat zeroed by the caller): the weight
 * gradient of ONE sample contracted with the weights IS that sum.  only_if (kmh_channel_stats, kmh_gn_bwd_coeffs) gates
 * the direct path on the device: with only_if != NULL and *only_if == 0 those calls do nothing; *fallback is set to 1
 * (and nothing else written) when some gamma is exactly 0, where dgamma cannot be recovered from xhat. */
int kmh_gn_bwd_coeffs_fold(const double* dstats, const double* bhat, const float* gamma, const float* beta,
                           const float* mean_rstd, int N, int C, int G, double count, float* c123, float* dgamma,
                           float* dbeta, int* fallback, void* stream);
/* ---- a3: ConvNet blocks with InstanceNorm kept lazy (keymorph/layers.py:137-187, norm_type "instance"; keymorph/net.py:7-36):
 *      the next convolution's loader applies IN + ReLU to the RAW (max-pooled raw) output z, so InstanceNorm3d -> ReLU ->
 *      [MaxPool3d(2)] has no forward pass of its own; its autograd, for du at the pooled resolution, zhat = z*scale + shift,
 *      g = scatter(du) [zhat > 0]:  dz = c1 g + c2 z + c3  (c123 from kmh_gn_bwd_coeffs with G = C).
 *      kmh_in_bwd_stats: out (N,C,2) doubles = (sum g, sum g z) taken at du's resolution (z = the pooled raw tensor there). */
int kmh_in_bwd_stats(const float* du, const float* z, const float* scale, const float* shift, int N, long long V, int C,
                     double* out, void* ws, void* stream);
/*      no pooling between z and u: dz (N,V,C) = c1 du [zhat > 0] + c2 z + c3; dz may alias du; dz_scale2 | NULL = {S, 1/S} */
int kmh_in_bwd_apply(const float* du, const float* z, const float* scale, const float* shift, const float* c123, int N,
                     long long V, int C, float* dz, float* dz_scale2, void* stream);
/*      through MaxPool3d(2): du (N,D/2,H/2,W/2,C), winners of kmh_maxpool3d_fwd on the raw z (N,D,H,W,C) -> dz (N,D,H,W,C) */
int kmh_in_bwd_apply_pool(const unsigned char* argmax, const float* du, const float* z, const float* scale,
                          const float* shift, const float* c123, int N, int D, int H, int W, int C, float* dz,
                          float* dz_scale2, void* stream);

/* dx_scale2 (float[2], ZERO on entry)|NULL: also emits {S, 1/S}, the f16x3 range scale of dx (what
 * kmh_absmax_scale(dx) would return), so the consumer convolution's backward needs no extra pass over its incoming
 * gradient. */
int kmh_gn_bwd_apply(const float* dxn, const float* x, const float* c123, int N, long long V, int C,
                     int relu_mask, int accumulate, float* dx, float* dx_scale2, int out_blocked, void* stream);
int kmh_relu_mask(const float* dy, const float* y, long long n, float* dz, void* stream);
/* y = act(x*scale[n,c] + shift[n,c]) on (N,V,C): InstanceNorm3d(+ReLU) apply of keymorph/layers.py:165,183-185 */
int kmh_norm_apply(const float* x, const float* scale, const float* shift, int N, long long V, int C, int relu,
                   float* y, void* stream);

/* MaxPool3d(2) (buildingblocks.py:363, layers.py:176), NDHWC */
/* argmax (N,D/2,H/2,W/2,C) bytes | NULL: index 0..7 of each window's first maximum (scan order z, y, x), for the
 * backward */
int kmh_maxpool3d_fwd(const float* x, float* y, unsigned char* argmax, int N, int D, int H, int W, int C, void* stream);
/* dx = scatter(dy) [+ add]: the winner of each window from `argmax` (x may then be NULL: a full-resolution read less)
 * or by rescanning x; add (N,D,H,W,add_cstride >= C)|NULL is a second gradient of x summed in the same pass
 * (U-Net skip connection; may alias dx).  Odd D/H/W: the caller pre-fills the window-less trailing planes. */
int kmh_maxpool3d_bwd(const float* x, const unsigned char* argmax, const float* dy, const float* add, int add_cstride,
                      float* dx, int N, int D, int H, int W, int C, int out_blocked, void* stream);
/* MaxPool3d(2)'s backward written PRE-SPLIT for kmh_conv3d_fwd_bf(in_blocked = 2): dxs is (N, C/8, D*H*W + 1) records of 32
 * bytes (kmh_maxpool3d_bwd_split_bytes), dy_scale2 = {S, 1/S} the range scale of dy (a scatter keeps it); even D, H, W,
 * C % 8 == 0; autograd of max_pool3d (keymorph/unet3d/buildingblocks.py:321-380) in the consumer's operand format. */
size_t kmh_maxpool3d_bwd_split_bytes(int N, int D, int H, int W, int C);
int kmh_maxpool3d_bwd_split(const unsigned char* argmax, const float* dy, const float* dy_scale2, float* dxs, int N, int D,
                            int H, int W, int C, void* stream);
/* dx = scatter(dy) + [x > 0] (c1 dxn + c2 x + c3): the pooling backward summed with the skip connection's gradient whose
 * GroupNorm backward (c123 (N,C,3), kmh_gn_bwd_apply's coefficients) is applied on the fly -- autograd of max_pool3d plus
 * the decoder's skip (keymorph/unet3d/buildingblocks.py:363, 471-475) in one pass; even D, H, W, C % 4 == 0, dense
 * tensors; dx_scale2 | NULL receives {S, 1/S} for max |dx| */
int kmh_maxpool3d_bwd_lazy(const unsigned char* argmax, const float* dy, const float* dxn, const float* x, const float* c123,
                           float* dx, int N, int D, int H, int W, int C, float* dx_scale2, void* stream);
/* decoder join: out = cat(skip, nearest_upsample(low -> skip size)) (buildingblocks.py:471-475,568-582) */
int kmh_upcat_fwd(const float* skip, const float* low, float* out, int N, int D, int H, int W, int Cs, int Dl,
                  int Hl, int Wl, int Cl, void* stream);
/* dskip == NULL: only dlow is produced (the caller reads dout[..., :Cs] in place, see kmh_maxpool3d_bwd's add) */
int kmh_upcat_bwd(const float* dout, float* dskip, float* dlow, int N, int D, int H, int W, int Cs, int Dl, int Hl,
                  int Wl, int Cl, int accumulate_skip, void* stream);
/* (N,C,V) <-> (N,V,C) */
int kmh_layout_convert(const float* in, float* out, int N, long long V, int C, int to_ncdhw, void* stream);

/* final 1x1x1 conv (keymorph/unet3d/model.py:96-99,387-391): x NDHWC (N,V,Cin) -> y NCDHW (N,Cout,V) */
int kmh_pointwise_pack(const float* w, float* wt, int Cout, int Cin, void* stream);
int kmh_pointwise_fwd(const float* x, const float* wt, const float* bias, float* y, int N, long long V, int Cin,
                      int Cout, void* stream);
int kmh_pointwise_dgrad(const float* dy, const float* w, float* dx, int N, long long V, int Cin, int Cout,
                        void* stream);
size_t kmh_pointwise_wgrad_ws_bytes(int N, long long V, int Cin, int Cout);
int kmh_pointwise_wgrad(const float* dy, const float* x, float* dw, float* dbias, int N, long long V, int Cin,
                        int Cout, int accumulate, void* ws, void* stream);

/* Fused keypoint head: final 1x1x1 conv + bias -> ReLU -> center of mass (keymorph/unet3d/model.py:387-391 +
 * keymorph/layers.py:92-134) without materialising the (N,K,D,H,W) heat-map; the backward recomputes the logits.
 * feat (N,D,H,W,Cin) NDHWC with Cin <= 64, w (Cout,Cin), bias (Cout)|NULL, pts (N,Cout,3) ij order,
 * sums (N,Cout,4) = {m, mz, my, mx} kept for the backward. */
size_t kmh_headcom_fwd_ws_bytes(int N, long long V, int Cout);
size_t kmh_headcom_bwd_ws_bytes(int N, long long V, int Cin, int Cout);
int kmh_headcom_fwd(const float* feat, const float* w, const float* bias, float* pts, float* sums, float* sq, int N, int D,
                    int H, int W, int Cin, int Cout, void* ws, void* stream);
/* dpower (N,Cout)|NULL: gradient of the loss w.r.t. sums[..., 0] = sum relu(h) (keypoint weighting by power,
 * keymorph/model.py:96-109), added to the center-of-mass gradient inside the same pass. */
/* mask_dfeat != 0: dfeat is zeroed where feat <= 0 (feat is a ReLU output, so its producer's backward receives the
 * gradient already masked and skips its own mask pass). */
int kmh_headcom_bwd(const float* dpts, const float* dpower, const float* feat, const float* w, const float* bias,
                    const float* sums, float* dfeat, float* dw, float* dbias, int N, int D, int H, int W, int Cin,
                    int Cout, int mask_dfeat, void* ws, void* stream);
/* split-operand MFMA arithmetic (terms = 2: scaled f16x3, the default of the Python host; terms = 3: bf16x6), same
 * contracts; Cin % 4 == 0 */
size_t kmh_headcom_fwd_bf_ws_bytes(int N, long long V, int Cout, int terms);
size_t kmh_headcom_bwd_bf_ws_bytes(int N, long long V, int Cin, int Cout, int terms);
/* scales_out (float[4]) | NULL: the {S, 1/S} range scales of feat and w measured by this call (terms = 2); handed back
 * as scales_in, the backward skips its two measuring passes.  dfeat_scale2 (float[2], ZERO on entry) | NULL: also emits
 * the range scale of dfeat (what kmh_absmax_scale(dfeat) would return) for the consumer convolution's backward.
 * mask (kmh_headcom_mask_words(N, D, H, W, Cout) 32-bit words; 0 words = this geometry has no mask path) | NULL: the
 * forward also stores [h > 0], 1 bit per (voxel, keypoint channel) -- the ReLU of keymorph/layers.py:99 -- and a backward
 * handed the same buffer skips recomputing the logits (half its matrix work); with NULL the backward recomputes them. */
size_t kmh_headcom_mask_words(int N, int D, int H, int W, int Cout);
int kmh_headcom_fwd_bf(const float* feat, const float* w, const float* bias, float* pts, float* sums, float* sq,
                       float* scales_out, int N, int D, int H, int W, int Cin, int Cout, int terms, unsigned* mask, void* ws,
                       void* stream);
int kmh_headcom_bwd_bf(const float* dpts, const float* dpower, const float* feat, const float* w, const float* bias,
                       const float* sums, float* dfeat, float* dw, float* dbias, int N, int D, int H, int W, int Cin,
                       int Cout, int terms, int mask_dfeat, const float* scales_in, float* dfeat_scale2,
                       const unsigned* mask, void* ws, void* stream);

/* caller-side optimizer (scripts/run.py:439 torch.optim.Adam): one fused launch over a flat buffer.
 * g is multiplied by grad_scale first (1/world_size after the RCCL sum all-reduce). */
int kmh_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                  float eps, int step, float grad_scale, void* stream);

/* ---- brain extraction (keymorph/model.py:533-659, notebooks/[B] Brain Extraction.ipynb) ---- */
/* Trilinear resize with PyTorch's align_corners=False semantics.  channels_last == 0: (N,C,D,H,W) storage, else (N,D,H,W,C);
 * the two layouts give bit-identical values.  tz / ty / tx: per-axis device tables of 3 * out ints built by the host with
 * separately rounded fp32 operations: taps i0[out], taps i1[out], weights lam[out] (float bits).  The backward is the exact
 * transpose written as a gather (no float atomics): rz / ry / rx hold 2 * in ints, the first and the last output index that
 * references each input index (first > last: none).  Tensors of 2^31 elements or more: -22. */
int kmh_resize_trilinear3d_fwd(const float* x, float* y, int N, int C, int D, int H, int W, int Do, int Ho, int Wo,
                               const int* tz, const int* ty, const int* tx, int channels_last, void* stream);
int kmh_resize_trilinear3d_bwd(const float* gy, float* gx, int N, int C, int D, int H, int W, int Do, int Ho, int Wo,
                               const int* tz, const int* ty, const int* tx, const int* rz, const int* ry, const int* rx,
                               int channels_last, void* stream);
/* Connected components with 26-neighbour connectivity of N binary masks (N,D,H,W) bytes: labels (int32) = 1 + the
 * raster-order linear index of the component's first voxel, 0 = background.  kmh_clean_mask3d: out = 1 where the voxel's
 * component has size / (largest size of its sample) > threshold (division in double).  info (N + 1 ints) | NULL: the largest
 * component size per sample (kmh_clean_mask3d only), then a flag set when a mask value other than 0 / 1 was seen. */
size_t kmh_components3d_ws_bytes(int N, int D, int H, int W);
int kmh_components3d(const unsigned char* mask, int* labels, int N, int D, int H, int W, int* info, void* ws, void* stream);
int kmh_clean_mask3d(const unsigned char* mask, unsigned char* out, int N, int D, int H, int W, double threshold, int* info,
                     void* ws, void* stream);

/* Direct fp32 3x3x3 convolutions (padding 1, NDHWC, exact fp32 FMAs) for thin layers the split-operand kernels are not built
 * for (Simple_Unet: 1 -> 4, 4 -> 8, 8 -> 1, 1 -> 1 and the transposed pairs).  kmh_conv3d_thin_ok(Cin, Cout): the forward /
 * data-gradient kernel serves a LAUNCH with these input / output channels (Cin <= 8, Cout in {1, 4, 8, 16});
 * kmh_conv3d_thin_wgrad_ok: the weight gradient serves the layer (27 Cin Cout + Cout <= 1024).
 * fwd: y = conv(x, w (Cout,Cin,3,3,3)) + bias|NULL, ReLU if relu_out.  dgrad: dx (..,Cin) from dz (..,Cout) and the layer's w;
 * dzmask (dz's shape)|NULL: the layer's ReLU output, dz counts as 0 where it is not > 0.  wgrad: dw and db|NULL; partial sums go
 * through ws and a fixed-order second pass (no float atomics: repeat calls are bit-identical). */
int kmh_conv3d_thin_ok(int Cin, int Cout);
int kmh_conv3d_thin_wgrad_ok(int Cin, int Cout);
int kmh_conv3d_thin_fwd(const float* x, const float* w, const float* bias, float* y, int N, int D, int H, int W, int Cin,
                        int Cout, int relu_out, void* stream);
int kmh_conv3d_thin_dgrad(const float* dz, const float* dzmask, const float* w, float* dx, int N, int D, int H, int W, int Cin,
                          int Cout, void* stream);
size_t kmh_conv3d_thin_wgrad_ws_bytes(int N, int D, int H, int W, int Cin, int Cout);
int kmh_conv3d_thin_wgrad(const float* x, const float* dz, const float* dzmask, float* dw, float* db, int N, int D, int H,
                          int W, int Cin, int Cout, void* ws, void* stream);

/* ---- sampling grids as transforms (keymorph_amd/fields.py) ----
 * A grid (N,D,H,W,3) is xyz, normalised, align_corners=False, and as a function of space its own trilinear interpolant with
 * border clamping (what kmh_grid_sample3d_fwd does to any volume).  Ids[k,j,i] = ((2i+1)/W - 1, (2j+1)/H - 1, (2k+1)/D - 1).
 * A lattice of 2^31 voxels or more, or a gathered grid of 2^30 floats or more per sample: -22. */
int kmh_field_identity(float* out, int N, int D, int H, int W, void* stream);
/* out (N,Do,Ho,Wo,3) = then (N,D,H,W,3) interpolated at first (N,Do,Ho,Wo,3): bit-identical to sampling the (N,3,D,H,W) copy
 * of `then` with kmh_grid_sample3d_fwd, read channels-last instead. */
int kmh_field_compose(const float* first, const float* then, float* out, int N, int Do, int Ho, int Wo, int D, int H, int W,
                      void* stream);
/* out[w] = c with grid(c) = Ids[w]: per-voxel Newton steps from c0 = start (N,3,4) applied to Ids[w], each limited to one voxel
 * per axis and clamped to [-1, 1], until max |residual| <= tol or max_iters steps; a near-singular Jacobian steps through the
 * linear part of `start`.  converged (N,D,H,W) bytes; unconverged (N) = voxels with converged == 0; max_residual (N) over the
 * converged voxels; iterations (N) | NULL = Newton steps taken.  A voxel that meets a non-finite value ends flagged, finite and
 * inside [-1, 1].  Every axis >= 2.  ws = kmh_field_invert_ws_bytes(). */
size_t kmh_field_invert_ws_bytes(int N, int D, int H, int W);
int kmh_field_invert(const float* grid, const float* start, float* out, unsigned char* converged, long long* unconverged,
                     float* max_residual, long long* iterations, int N, int D, int H, int W, float tol, int max_iters, void* ws,
                     void* stream);
/* disp (N,3,D,H,W), channels (z,y,x), in voxels = (grid - Ids) * size / 2 (what kmh_jacobian_det reads), and back. */
int kmh_field_to_displacement(const float* grid, float* disp, int N, int D, int H, int W, void* stream);
int kmh_field_from_displacement(const float* disp, float* grid, int N, int D, int H, int W, void* stream);

/* ---- free-form deformation: a grid from a lattice of cubic B-spline control points (csrc/bspline.hip states the definition) ----
 * ctrl (N,3,Cz,Cy,Cx), channel k = displacement of grid component k (x,y,z), normalised; an axis of S voxels and C >= 4 control
 * points has C - 3 cells over [-1, 1].  out (N,D,H,W,3) = base + the spline, base = Ids of the fields section (mat NULL) or what
 * kmh_affine_grid_fwd writes for mat (N,3,4).  kmh_bspline_grid_bwd: dctrl = the transposed operator applied to dgrid, no
 * atomics, bit-identical from run to run, a batch equals its samples; ws = kmh_bspline_grid_ws_bytes() bytes.
 * -22: a C below 4, an empty shape, N outside 1..65535, 2^31 voxels or control points per channel or more. */
int kmh_bspline_grid_fwd(const float* ctrl, const float* mat, float* out, int N, int D, int H, int W, int Cz, int Cy, int Cx,
                         void* stream);
size_t kmh_bspline_grid_ws_bytes(int N, int D, int H, int W, int Cz, int Cy, int Cx);
int kmh_bspline_grid_bwd(const float* dgrid, float* dctrl, int N, int D, int H, int W, int Cz, int Cy, int Cx, void* ws,
                         void* stream);
/* out[n] = sum over the three lattice axes of the mean of (q[i-1] - 2 q[i] + q[i+1])^2 over that axis' differenced tensor,
 * q (N,3,Cz,Cy,Cx) with every C >= 4; dq = gout[n] d out[n] / dq.  Fixed-order sums; ws = kmh_bspline_bending_ws_bytes(N). */
size_t kmh_bspline_bending_ws_bytes(int N);
int kmh_bspline_bending_fwd(const float* q, float* out, int N, int Cz, int Cy, int Cx, void* ws, void* stream);
int kmh_bspline_bending_bwd(const float* q, const float* gout, float* dq, int N, int Cz, int Cy, int Cx, void* stream);

/* ---- diffeomorphic grids: a stationary velocity field exponentiated by scaling and squaring (csrc/svf.hip states the definition) ---- */
/* kmh_bspline_disp_fwd: out (N,D,H,W,3) = the spline of kmh_bspline_grid_fwd WITHOUT its base (same limits, same -22);
 * kmh_bspline_grid_bwd is its transpose too.
 * Displacements u, first, add, out, g, du and grids are (N,D,H,W,3) float32 contiguous, xyz, normalised, on the voxel-centre lattice;
 * N in [1, 65535] and D*H*W*3 < 2^30 (one buffer descriptor per sample), else -22 before anything is launched.
 * kmh_svf_compose: out[w] = add[w] + U(first[w]), U = the border-clamped trilinear interpolant of u (the sampler's coordinate,
 *   clamp and NaN rule).  first == NULL: first = Ids + u, add = u -- one squaring step, bit-identical to sampling u at
 *   identity + u and adding u.  out must not be u.
 * kmh_svf_finish_fwd: out = Ids + u (mat NULL), else kmh_affine_grid_fwd's grid + L (s * u), L = mat[:, :3], s = S / (S - 1) per
 *   axis (every axis >= 2).  out may be u.  kmh_svf_finish_bwd: du = the transpose applied to dgrid; amax_out (N unsigned, zeroed by
 *   the caller, or NULL) receives the bits of the largest finite |du| of each sample.
 * kmh_svf_square_bwd: the transpose of a squaring step, du from g (du may be g): the per-voxel part directly, the scattered part
 *   in 64-bit fixed point with integer atomics, scaled per sample by amax_in (N unsigned: what kmh_svf_finish_bwd or the previous
 *   call published) -- order independent, so runs repeat bit for bit and a batch equals its samples.  amax_out as above.
 *   ws: kmh_svf_square_bwd_ws_bytes bytes (32 per voxel), cleared by the call. */
int kmh_bspline_disp_fwd(const float* ctrl, float* out, int N, int D, int H, int W, int Cz, int Cy, int Cx, void* stream);
int kmh_svf_compose(const float* u, const float* first, const float* add, float* out, int N, int D, int H, int W, void* stream);
int kmh_svf_finish_fwd(const float* u, const float* mat, float* out, int N, int D, int H, int W, void* stream);
int kmh_svf_finish_bwd(const float* dgrid, const float* mat, float* du, unsigned* amax_out, int N, int D, int H, int W,
                       void* stream);
size_t kmh_svf_square_bwd_ws_bytes(int N, int D, int H, int W);
int kmh_svf_square_bwd(const float* u, const float* g, float* du, const unsigned* amax_in, unsigned* amax_out, int N, int D, int H,
                       int W, void* ws, void* stream);

/* ---- dense displacement fields as a transform model (csrc/dense.hip states the definitions) ---- */
/* disp, delta, ddisp, out: PLANAR (N,3,D,H,W) float32 contiguous, channels (z, y, x), voxels of their own lattice
 * (kmh_field_to_displacement's convention); grid, dgrid (N,D,H,W,3); N in [1, 65535] and D*H*W*3 < 2^30, else -22 before anything is
 * launched.
 * kmh_disp_grid_fwd: grid = Ids + u, u = disp over S / 2 per axis in xyz (mat NULL: bit-identical to kmh_field_from_displacement),
 *   else kmh_affine_grid_fwd's grid + L (s * u) as kmh_svf_finish_fwd (every axis >= 2).  kmh_disp_grid_bwd: its transpose in disp.
 * kmh_disp_step_scale: out[n] = step / max_w |delta[n, :, w]|_2 over the voxels whose squared norm is finite, 0 where that maximum
 *   is 0; an integer max on float bits, so runs repeat bit for bit and a batch equals its samples.  Nothing is read back.
 * kmh_disp_update: out[n, :, w] = d[w] + U_n(Ids[w] + d[w] over S / 2), d = delta * scale[n] (scale (N) in device memory, or NULL:
 *   delta), U_n the border-clamped trilinear interpolant of disp[n] (the sampler's coordinate, clamp and NaN rule); every product
 *   and sum rounded on its own.  out must not be disp. */
int kmh_disp_grid_fwd(const float* disp, const float* mat, float* grid, int N, int D, int H, int W, void* stream);
int kmh_disp_grid_bwd(const float* dgrid, const float* mat, float* ddisp, int N, int D, int H, int W, void* stream);
int kmh_disp_step_scale(const float* delta, float step, float* out, int N, int D, int H, int W, void* stream);
int kmh_disp_update(const float* disp, const float* delta, const float* scale, float* out, int N, int D, int H, int W,
                    void* stream);

/* ---- local normalised cross-correlation (csrc/lncc.hip states the definition) ---- */
/* a, b: (N, D, H, W) float32 contiguous, fewer than 2^31 voxels per sample; window odd in [3, 15], truncated at the border.
 * out[n] = mean over the voxels of cross^2 / (va vb + eps) of the window sums.  kmh_lncc_bwd: da = gout[n] d out[n] / da, db
 * likewise, either may be NULL.  ws: kmh_lncc_ws_bytes bytes (one float per tile and sample, and the backward's five coefficient
 * fields: 2.5 times the two inputs); the backward reads nothing the forward left there.  No atomics: runs repeat bit for bit and
 * a batch equals its samples.  -22 for an even or out-of-range window, N < 1, an empty volume or a null pointer. */
size_t kmh_lncc_ws_bytes(int N, int D, int H, int W, int window);
int kmh_lncc_fwd(const float* a, const float* b, int N, int D, int H, int W, int window, float eps, float* out, void* ws,
                 void* stream);
int kmh_lncc_bwd(const float* a, const float* b, const float* gout, int N, int D, int H, int W, int window, float eps,
                 float* da, float* db, void* ws, void* stream);

/* ---- MIND-SSC, the self-similarity context descriptor as a similarity (csrc/mind.hip states the definition) ---- */
/* a, b: (N, D, H, W) float32 contiguous, fewer than 2^31 voxels per sample; radius and dilation in 1..3.  bounds (N, 2, 2) =
 * [a or b][lo or hi], the clamp of the descriptor's variance, constants of the call: kmh_mind_bounds writes (1e-3, 1e3) x each
 * sample's mean of it.  out[n] = mean over the voxels and the 12 channels of (M_c(a) - M_c(b))^2, >= 0, lower is better.
 * kmh_mind_bwd: da = gout[n] d out[n] / da, db likewise, either may be NULL.  ws: kmh_mind_ws_bytes bytes (two floats per tile
 * and sample, and the backward's 18 fields of one side: 72 bytes per voxel); the backward reads nothing the forward left there.
 * No atomics: runs repeat bit for bit and a batch equals its samples.  -22 for a radius or dilation outside 1..3, N < 1, an
 * empty volume, 2^31 voxels or more, or a null pointer; kmh_mind_ws_bytes is 0 for those. */
size_t kmh_mind_ws_bytes(int N, int D, int H, int W, int radius, int dilation);
int kmh_mind_bounds(const float* a, const float* b, int N, int D, int H, int W, int radius, int dilation, float* bounds,
                    void* ws, void* stream);
int kmh_mind_fwd(const float* a, const float* b, const float* bounds, int N, int D, int H, int W, int radius, int dilation,
                 float* out, void* ws, void* stream);
int kmh_mind_bwd(const float* a, const float* b, const float* bounds, const float* gout, int N, int D, int H, int W, int radius,
                 int dilation, float* da, float* db, void* ws, void* stream);

/* ---- cubic B-spline resampling (csrc/cubic.hip states the definition) ----
 * x, coef (N,C,D,H,W); grid (N,Do,Ho,Wo,3) xyz in the convention of kmh_grid_sample3d_fwd (border, align_corners=False, the same
 * fp32 source coordinate, clamp mask and NaN rule).  kmh_cubic_prefilter: coef = the cubic B-spline coefficients of x, separably
 * along W, H, D with whole-sample mirror ends (an axis of length 1 is left alone).  kmh_cubic_sample_fwd:
 * out (N,C,Do,Ho,Wo) = the spline of coef at grid (64 taps, mirrored at the ends; it overshoots and is not clamped).
 * kmh_cubic_sample_bwd_grid: dgrid (N,Do,Ho,Wo,3) = d(out)/d(grid) contracted with gout (N,C,Do,Ho,Wo); 0 on a clamped axis, 0
 * on all three for a voxel with a NaN coordinate.  There is no gradient with respect to the volume.  No atomics: runs repeat bit
 * for bit and a batch equals its samples.  -22 for a null pointer, an empty shape, a channel plane of 2^29 voxels or more or
 * N > 65535. */
int kmh_cubic_prefilter(const float* x, float* coef, int N, int C, int D, int H, int W, void* stream);
int kmh_cubic_sample_fwd(const float* coef, const float* grid, float* out, int N, int C, int D, int H, int W, int Do, int Ho,
                         int Wo, void* stream);
int kmh_cubic_sample_bwd_grid(const float* coef, const float* grid, const float* gout, float* dgrid, int N, int C, int D, int H,
                              int W, int Do, int Ho, int Wo, void* stream);

/* ---- Gaussian smoothing and its transpose (csrc/gauss.hip states the definition) ----
 * x, out, gout, dx (N,C,D,H,W) float32.  Per axis a radius r (rz, ry, rx; 0 = the axis is not touched) and HOST pointers: w* to
 * the half-kernel w[0..r] (w[|k|], normalised over k = -r..r), t* to the tail sums t[i] = sum_{k >= i} w[k], i = 0..r (the
 * transpose only); a pointer may be NULL where its radius is 0.  The launcher copies them into kernel arguments by value: no
 * host-to-device copy.  kmh_gauss_fwd: out[i] = sum_k w[k] x[clamp(i + k, 0, n - 1)] along W, then H, then D.  kmh_gauss_bwd:
 * dx = the transposed operator applied to gout, a gather, along D, then H, then W.  ws: kmh_gauss_ws_bytes(...) bytes of
 * scratch (0 with fewer than two active axes; ws may then be NULL).  out must not alias x (nor dx gout), ws neither.  No
 * atomics: runs repeat bit for bit and a batch equals its samples.  -22 (kmh_gauss_ws_bytes: 0) for a null pointer, an empty
 * shape, a radius outside 0..32, a channel plane of 2^29 voxels or more or N C > 65535. */
size_t kmh_gauss_ws_bytes(int N, int C, int D, int H, int W, int rz, int ry, int rx);
int kmh_gauss_fwd(const float* x, float* out, void* ws, int N, int C, int D, int H, int W, int rz, int ry, int rx,
                  const float* wz, const float* wy, const float* wx, void* stream);
int kmh_gauss_bwd(const float* gout, float* dx, void* ws, int N, int C, int D, int H, int W, int rz, int ry, int rx,
                  const float* wz, const float* wy, const float* wx, const float* tz, const float* ty, const float* tx,
                  void* stream);

/* ---- label maps through a grid by trilinear vote (csrc/label_warp.hip states the definition) ----
 * lab (N,C,D,H,W): integer label maps, every channel a map of its own, of elem_bytes 1 (is_signed 0: uint8, bool) or 2 / 4 / 8
 * (is_signed 1); grid (N,Do,Ho,Wo,3) in the convention of kmh_grid_sample3d_fwd.  out (N,C,Do,Ho,Wo), same element type: per
 * voxel the label l with the largest S_l = the bilinear sample of the channel [lab == l] (same corners, same fma chain, so
 * out = argmax over the one-hot channels of kmh_grid_sample3d_fwd bit for bit), the smallest such label on a tie; weight (same
 * shape, float32, or NULL) = that S_l.  One launch, no atomics.  -22 for a null pointer, an empty shape, another element type,
 * a channel plane of 2^29 voxels or more or N C > 65535. */
int kmh_warp_labels(const void* lab, int elem_bytes, int is_signed, const float* grid, void* out, float* weight, int N, int C,
                    int D, int H, int W, int Do, int Ho, int Wo, void* stream);

/* ---- Dice on integer label maps (csrc/label_dice.hip; element types as kmh_warp_labels) ----
 * kmh_label_presence_int: kmh_label_presence for the four widths; flags (nflags + 1 ints) is only ever set, so several maps can
 * share it.  kmh_label_pair_counts: counts (3 * nlab uint64, zeroed by the caller) = {|x = l|, |y = l|, |x = l and y = l|} over
 * the n ids of x and y, l = slot_of[id] for ids in [0, nids); an id outside the table or a slot >= nlab is not counted;
 * nlab <= 4096. */
int kmh_label_presence_int(const void* seg, int elem_bytes, int is_signed, long long n, int nflags, int* flags, void* stream);
int kmh_label_pair_counts(const void* x, const void* y, int elem_bytes, int is_signed, long long n,
                          const unsigned short* slot_of, int nids, int nlab, unsigned long long* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KEYMORPH_HIP_H */
