/*
 * mpn.h — C ABI of libmpn_hip.so: the MI355X (gfx950) kernels behind the MultiPoseNet hot path.
 *
 * Boundary rules: extern "C", plain pointers + sizes, no torch types.  Every entry
 * point enqueues work on the caller's stream (`hipStream_t` passed as void*), never allocates,
 * never synchronises (except where stated), and returns 0 on success or the hipError_t code /
 * a negative MPN_E* code on a bad argument.  All tensors are device pointers unless stated.
 *
 * Tensor model: activations are NHWC ("pixel-major"): element (b, h, w, c) of a tensor lives at
 *     base + b*sB + (h*W + w)*sP + c            (strides in ELEMENTS, channel stride 1)
 * Internal tensors keep their channel count padded to a multiple of 32 (pad lanes hold zeros) so
 * every 64-byte K-chunk load is in bounds and 16-byte aligned.  dtype codes: 0 = f32, 1 = bf16, 2 = f16.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference).
 */
#ifndef MPN_H_
#define MPN_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPN_F32 0
#define MPN_BF16 1
#define MPN_F16 2      /* IEEE half: same kernels, v_mfma_f32_16x16x32_f16 (BASELINE config 5 inference arithmetic) */

#define MPN_E_BADARG (-2)
#define MPN_E_UNSUPPORTED (-3)

/* ---------------------------------------------------------------------------------------------
 * Convolution (implicit GEMM on MFMA).  Replaces every nn.Conv2d / nn.Linear call site of
 * network/fpn.py:14-26,42-76, network/posenet.py:36-46,78-89,133-135,165-186 (forward) and the
 * autograd backward torch derives for them (training/trainer.py:251).
 * -------------------------------------------------------------------------------------------*/
typedef struct MpnConvParams {
    const void* x;        /* gathered operand: fwd = input activations, dgrad = dY                */
    const void* w;        /* fwd: [Cout][R][S][Cin]; dgrad: [Cout'][R][S][Cin'] = Wt (see below)    */
    void* y;              /* output tensor                                                        */
    const float* bias;    /* optional [Cout] f32                                                  */
    const float* scale;   /* optional [Cout] f32 per-channel multiplier applied before bias       */
    const void* res;      /* optional residual (same element type as y)                           */
    const uint8_t* res_mask; /* optional, res_mode 1 only: the residual is multiplied by these mask bits (layout of bnb_mask /
                              * mpn_bn_act_forward's mask, dense [pixels][Cout_store / V]) before it is added — the gradient of
                              * relu(bn3(.) + shortcut) w.r.t. the shortcut is dz * (z > 0): the dgrad launch that completes the
                              * shortcut's gradient reads dz and the bits instead of a materialised copy (network/fpn.py:30-33)  */
    float* stats;         /* optional [tilesP][Cout][2] per-tile (sum, sumsq) partials (BN train) */
    int64_t x_sB, x_sH, x_sW;
    int64_t y_sB, y_sP;
    int64_t res_sB, res_sP;
    int32_t B, H, W, Cin; /* source dims; Cin = contraction channels per tap (mult. of 64 bytes)  */
    int32_t Ho, Wo, Cout, Cout_store; /* output dims; channels [Cout, Cout_store) are written 0   */
    int32_t R, S, stride, pad;
    int32_t mode;         /* 0: hi = ho*stride - pad + r ; 1 (dgrad): hi = (ho + pad - r)/stride   */
    int32_t act;          /* 0 none, 1 relu, 2 sigmoid (both before the residual stage), 3 relu AFTER a same-size
                           * residual add: with scale/bias = folded BatchNorm this is a whole Bottleneck tail
                           * relu(bn3(conv3(x)) + shortcut) (network/fpn.py:30-33) in one launch (frozen statistics) */
    int32_t res_mode;     /* 0 none, 1 same size, 2 nearest-upsampled from [res_H, res_W]          */
    int32_t res_H, res_W;
    int32_t accumulate;   /* y = y + result (act must be 0)                                       */
    int32_t dtype;        /* element type of x, w                                                 */
    int32_t out_f32;      /* 1: y (and res) are f32 even when dtype is bf16                       */
    /* Pyramid mode (nseg > 0): ONE launch applies the same weights to nseg <= MPN_MAX_SEG feature maps of different sizes —
     * the shared RetinaNet towers of network/posenet.py:33-117,327-328, which the reference runs level by level.  Level l
     * has its own dense tensors seg_x[l] / seg_y[l] ([B][seg_H][seg_W][channels], same channel strides x_sW / y_sP as the
     * single-tensor fields; stride 1, output size = input size) and owns the pixel tiles [seg_tile0[l], seg_tile0[l+1]);
     * a workgroup never straddles two levels.  x, y, H, W, Ho, Wo, x_sB, x_sH, y_sB are ignored in this mode.           */
    int32_t nseg;
    int32_t seg_H[5], seg_W[5];
    int32_t seg_tile0[6];
    const void* seg_x[5];
    void* seg_y[5];
    /* BatchNorm-backward statistics in the epilogue (bnb_partial != NULL; dgrad launches): the tensor this launch completes
     * is dz, the gradient w.r.t. the OUTPUT of a BatchNorm(+ReLU) layer z = act(bn(y_bn) [+ residual]) (network/fpn.py:28-34).
     * With g = dz * (z > 0) the launch also writes, per pixel tile, (sum g, sum g * xhat), xhat = (y_bn - mean) * invstd —
     * exactly what mpn_bn_bwd_reduce would produce in an extra pass over dz, y_bn (and z): bnb_partial [tiles][Cout][2] with
     * tiles = mpn_conv_stats_tiles(), consumed by mpn_bn_bwd_finalize(partial, tiles, ...).  bnb_y / bnb_z have the geometry,
     * element type and strides of y; bnb_z == NULL with bnb_relu: the mask is recomputed as y_bn*bnb_scale + bnb_shift > 0 (valid
     * when the forward had no residual input).  Statistics use the values as stored (after rounding to the element type).    */
    const void* bnb_y;
    const void* bnb_z;
    const uint8_t* bnb_mask; /* alternative to bnb_z: the ReLU mask as bits written by mpn_bn_act_forward(mask=...) — one byte per
                              * 16-byte chunk of z (8 channels of a 16-bit type, 4 of f32), bit k = (z[chunk*V + k] > 0), dense
                              * [pixels][Cout_store / V]; 1/16 of z's bytes.  Takes precedence over bnb_z.                       */
    const float* bnb_mean;
    const float* bnb_invstd;
    const float* bnb_scale;
    const float* bnb_shift;
    float* bnb_partial;
    int32_t bnb_relu;
    /* In-launch finalize (fin_counters != NULL, together with `stats` or `bnb_partial`): the LAST workgroup to finish a tile
     * of output channels reduces that tile's per-pixel-tile partials (fixed order, double precision — deterministic whatever
     * the arrival order) and does the work of mpn_bn_finalize_train (stats: fin_out = [4][Cout] mean, invstd, scale, shift;
     * running statistics updated when fin_rm / fin_rv are given) or of mpn_bn_bwd_finalize (bnb_partial: fin_dgamma += ,
     * fin_dbeta += , fin_out = [3][Cout] k1, k2, k3 with fin_train selecting batch-statistics or frozen coefficients; mean /
     * invstd are bnb_mean / bnb_invstd).  fin_counters: one zeroed uint32 per output-channel tile (64 entries); the launch leaves
     * them zero again.  Launches sharing a counter array must be ordered (one stream).           */
    /* Virtual channel concatenation of the gathered operand (kseg_n > 0; 3x3 / stride 1 / pad 1 launches with 16-bit operands):
     * the input is cat_s(nearest_upsample(kseg_x[s])) over kseg_n <= 4 segments of kseg_c channels each (Cin = kseg_n * kseg_c) —
     * torch.cat((up8(q5), up4(q4), up2(q3), q2), 1) feeding conv2 (network/posenet.py:311-315) — and is never materialised:
     * segment s is the dense tensor [B][H >> kseg_shift[s]][W >> kseg_shift[s]][kseg_c] and pixel (h, w) of the virtual input reads
     * its pixel (h >> shift, w >> shift).  H, W are the virtual (output) size; x, x_sB, x_sH, x_sW are ignored.            */
    int32_t kseg_n, kseg_c;
    int32_t kseg_shift[4];
    const void* kseg_x[4];
    uint32_t* fin_counters;
    const float* fin_gamma;
    const float* fin_beta;
    float* fin_rm;
    float* fin_rv;
    float* fin_out;
    float* fin_dgamma;
    float* fin_dbeta;
    double fin_count;
    float fin_momentum, fin_eps;
    int32_t fin_train;
    /* Parity classes of a stride-2 input gradient (y_step == 2; round 4).  dx[h][w] of a 3x3 / stride 2 / pad 1 convolution only receives
     * the taps r = (h + 1) mod 2 (+ 2), s likewise: of the nine taps 1, 2, 2 or 4 are live, depending on the parities (a, c) of (h, w) — the
     * gather form (mode 1, stride 2) multiplies the other 6.75 of 9 with zeros.  One launch per class computes
     *   dx[b][2 i + a][2 j + c] = sum_{t_r <= a, t_s <= c} dy[b][i + t_r][j + t_s] . W[a + 1 - 2 t_r][c + 1 - 2 t_s]
     * as a FORWARD gather (mode 0, stride 1, pad 0, R = 1 + a, S = 1 + c) over dy whose output pixel (i, j) is stored at
     * (y_step i + y_oh, y_step j + y_ow) of the dense [B][y_H][y_W] tensor y (and of every output-shaped operand: accumulate, bnb_y,
     * bnb_mask), and whose filter tap (t_r, t_s) is tap wtap0 + t_r wtap_dr + t_s wtap_ds of a weight tensor with w_taps taps per output
     * channel ([Cout][w_taps][Cin]).  Ho, Wo = the class grid (ceil((y_H - a) / 2), ceil((y_W - c) / 2)); rows of dy past its end read zeros.
     * Extended epilogue; not combined with nseg, kseg_n, res, fin_counters, stats, out_f32.  (torch.nn.Conv2d(stride=2) backward:
     * network/layers.py, the first Bottleneck of layer2-4; posenet.py P6 / P7.)                                                        */
    int32_t y_step, y_oh, y_ow, y_H, y_W;
    int32_t w_taps, wtap0, wtap_dr, wtap_ds;
} MpnConvParams;
#define MPN_MAX_SEG 5

/* number of pixel tiles (rows of `stats`) mpn_conv_forward will use for this problem */
int mpn_conv_stats_tiles(const MpnConvParams* p);
/* Host only (no HIP call): writes the NUL-terminated name of the instantiation mpn_conv_forward will launch for p, as rocprofv3 prints it
 * without the trailing experiments-only profiling flag: conv_igemm[_s3]_kernel<bf16|_Float16|float, TC, 128, OUTF32, GENERAL, EXT> — TC the
 * output-channel rows of the tile (256 / 128 / 64 / 32); _s3 the shared-pixel-tile kernel (3x3, stride 1, pad 1, 16-bit operands, dense
 * input: the pixel tile of a kernel row lands once and serves its three taps); GENERAL / EXT the epilogue (an extended one is general).
 * It is the launcher's own routing decision, so it cannot disagree with the launch.  Returns the length of the name; MPN_E_BADARG for a
 * null argument, an unknown dtype or a cap that does not hold the name and its NUL; MPN_E_UNSUPPORTED where mpn_conv_forward has no
 * instantiation (an extended epilogue with out_f32). */
int mpn_conv_kernel_name(const MpnConvParams* p, char* buf, int cap);
int mpn_conv_forward(const MpnConvParams* p, void* stream);

typedef struct MpnWgradParams {
    const void* x;        /* forward input activations (gathered)                                 */
    const void* dy;       /* output gradient, dense pixel-major: dy[p*dy_sP + cout]               */
    float* dw;            /* [Cout][R][S][Cin] f32, ACCUMULATED into (dw += result)               */
    float* ws;            /* workspace, >= chunks * Cout*R*S*Cin floats when chunks > 1           */
    int64_t x_sB, x_sH, x_sW;
    int64_t dy_sP;
    int32_t B, H, W, Cin;
    int32_t Ho, Wo, Cout;
    int32_t R, S, stride, pad;
    int32_t dtype;
    int32_t chunks;       /* split of the B*Ho*Wo contraction; use mpn_conv_wgrad_chunks()        */
    float* db;            /* optional bias gradient [Cout] f32, ACCUMULATED into: sum over pixels of dy.  Served
                           * only by the bf16 LDS-DMA kernel (mpn_conv_wgrad_kernel_id & 1), where it costs one
                           * extra MFMA against a vector of ones per dY fragment; otherwise must be NULL          */
    float* db_ws;         /* workspace, >= chunks * Cout floats, when db != NULL and chunks > 1                    */
    /* Pyramid mode (nseg > 0, LDS-DMA kernel only): the contraction runs over the pixels of nseg feature maps that share the
     * weights (see MpnConvParams); level l = dense tensors seg_x[l] / seg_dy[l] of size [B][seg_H][seg_W][.] (stride 1, same
     * size in and out) and owns the pixel slices [seg_chunk0[l], seg_chunk0[l+1]) of seg_chunk_pixels pixels each.  Fill
     * chunks / seg_chunk0 / seg_chunk_pixels with mpn_conv_wgrad_seg_plan().                                              */
    int32_t nseg;
    int32_t seg_H[5], seg_W[5];
    int32_t seg_chunk0[6];
    int32_t seg_chunk_pixels;
    const void* seg_x[5];
    const void* seg_dy[5];
    /* Virtual channel concatenation of x (see MpnConvParams.kseg_*): LDS-DMA kernel with 128-channel cin tiles, kseg_c == 128 —
     * every workgroup's cin tile is one segment.  H, W are the virtual size; x, x_sB, x_sH, x_sW are ignored.              */
    int32_t kseg_n, kseg_c;
    int32_t kseg_shift[4];
    const void* kseg_x[4];
} MpnWgradParams;
/* tools/kloop_profile.py only: device buffer [workgroups][4 waves][8] of uint64 that the following 128 x 128-tile bf16 weight-gradient
 * launches fill with per-wave s_memtime cycle sums of their k-loop phases (own-DMA wait, barrier wait, DMA issue, fragment reads +
 * MFMA issue, whole loop, epilogue, k-steps, start stamp); NULL = off (production kernels contain none of this) */
int mpn_debug_wgrad_prof(void* buf);
/* the same for the 128-row bf16 forward / input-gradient launches (conv_igemm_kernel, conv_igemm_s3_kernel); synchronises the device */
int mpn_debug_igemm_prof(void* buf);

int mpn_conv_wgrad_chunks(const MpnWgradParams* p);
/* pyramid mode: chooses the slice length for the summed pixel count, writes p->chunks, p->seg_chunk0, p->seg_chunk_pixels;
 * returns the number of slices (or a negative error) */
int mpn_conv_wgrad_seg_plan(MpnWgradParams* p);
int mpn_conv_wgrad(const MpnWgradParams* p, void* stream);
/* first stage only (chunks > 1): the per-slice partial gradients go to ws (and db_ws) and the caller finishes with
 * mpn_conv_wgrad_reduce(p, stream) — lets a profiler bracket the MFMA kernel alone */
int mpn_conv_wgrad_partials(const MpnWgradParams* p, void* stream);
/* second stage (chunks > 1): db += the slices' bias partials (when db is set), dw += their weight partials — the reduction
 * mpn_conv_wgrad runs, same kernels and order, so the two-call path gives bit-identical dw and db */
int mpn_conv_wgrad_reduce(const MpnWgradParams* p, void* stream);
/* which kernel mpn_conv_wgrad launches for p: (tile_cin << 16) | (tile_cout << 4) | linear_x_addressing << 1 | uses_lds_dma
 * (bit 1: the instantiation for stride-1 same-extent convolutions over a dense x — halo predicate only, no per-lane address arithmetic) */
int mpn_conv_wgrad_kernel_id(const MpnWgradParams* p);
/* Host only: the name of the instantiation mpn_conv_wgrad / mpn_conv_wgrad_partials will launch for p, from the same routing decision as
 * the launch and the id above: conv_wgrad_dma[_lin|_seg][_f16|_f32]_kernel<TM, TN>, or conv_wgrad_kernel<T, TM, TN> where the LDS-DMA
 * kernel does not serve the launch.  Returns and errors as mpn_conv_kernel_name. */
int mpn_conv_wgrad_kernel_name(const MpnWgradParams* p, char* buf, int cap);

/* dst[i] (+)= sum_{c<chunks} ws[c*n + i]  — deterministic second stage of split reductions */
int mpn_reduce_partials(const float* ws, int chunks, int64_t n, float* dst, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Parameter preparation (once per step): master f32 [Cout][R][S][Cin] -> compute-dtype copies.
 * -------------------------------------------------------------------------------------------*/
int mpn_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
/* same for either 16-bit type (dtype = MPN_BF16 or MPN_F16) */
int mpn_cast_f32(const float* src, void* dst, int64_t n, int dtype, void* stream);
/* Wt[ci][r][s][co_pad] = W[co][r][s][ci] (co >= Cout -> 0); ci_pad rows beyond Cin are zero too */
int mpn_weight_transpose(const float* w, void* wt, int Cout, int RS, int Cin, int Cout_pad,
                         int dtype, void* stream);
/* all layers at once.  table[l] = {src offset in `arena` (floats), dst offset in `dst` (elements), Cout, RS, Cin, Cout_pad,
 * first block of the layer, ceil(Cin/32)} as int64; nblocks = sum over layers of ceil(Cin/32)*ceil(Cout_pad/32)*RS */
int mpn_weight_transpose_batched(const float* arena, void* dst, const int64_t* table, int nlayers, int64_t nblocks,
                                 int dtype, void* stream);
/* copy f32 [Cout][K] -> dtype [Cout][Kpad] zero padded (used for narrow-Cin / linear layers) */
int mpn_weight_pad_k(const float* w, void* dst, int Cout, int K, int Kpad, int dtype, void* stream);
/* stem 7x7x3: W[64][7][7][3] f32 <-> packed [64][7][32] (slot s*4+c, c<3, s<7; rest zero) */
int mpn_stem_pack_weight(const float* w, void* packed, int Cout, int dtype, void* stream);
int mpn_stem_unpack_wgrad(const float* dpacked, float* dw, int Cout, void* stream);
/* image NCHW f32 [B,3,H,W] -> zero-bordered NHWC4 [B][H+6][W+8][4] (pad 3 top/left) */
int mpn_stem_pack_image(const float* img, int64_t sB, int64_t sC, int64_t sH, int64_t sW, void* dst,
                        int B, int H, int W, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BatchNorm2d (network/fpn.py:15-26,43) in train / eval mode, fused with ReLU and residual add
 * (Bottleneck.forward, fpn.py:28-34).
 * -------------------------------------------------------------------------------------------*/
/* train: reduce conv-epilogue partials -> mean/invstd, scale/shift, update running stats */
int mpn_bn_finalize_train(const float* stats, int tiles, int C, int64_t count, const float* gamma,
                          const float* beta, float* running_mean, float* running_var, float momentum,
                          float eps, float* mean, float* invstd, float* scale, float* shift, void* stream);
/* eval / frozen: scale/shift from running statistics */
int mpn_bn_finalize_eval(int C, const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, float eps, float* mean, float* invstd,
                         float* scale, float* shift, void* stream);
/* z = act(y*scale + shift [+ res]);  all [P][Cs] dense pixel-major with pixel stride Cs.  mask (optional, with relu): the sign
 * bits of the STORED z, one byte per 16-byte chunk ([P][Cs / V], V = 8 for 16-bit types, 4 for f32; bit k = z[chunk*V + k] > 0) —
 * what the backward of relu(bn(.) + shortcut) (network/fpn.py:30-33) needs of z, at 1/16 of its bytes. */
int mpn_bn_act_forward(const void* y, const void* res, void* z, const float* scale, const float* shift,
                       int64_t P, int C, int Cs, int relu, int dtype, uint8_t* mask, void* stream);
/* backward, stage 1: g = dz * (z > 0 if relu); partial sums of g and g*xhat per channel.
 * With relu and z == NULL the mask is recomputed as (y*mask_scale + mask_shift) > 0 — the forward's own expression
 * (valid when the forward had no residual input), which saves reading z. */
int mpn_bn_bwd_reduce(const void* dz, const void* z, const void* y, const float* mean, const float* invstd,
                      const float* mask_scale, const float* mask_shift, float* partial, int chunks, int64_t P, int C, int Cs, int relu, int dtype, void* stream);
/* backward, stage 2: reduce partials; dgamma += , dbeta += (if non-null); coef [3][C] = k1,k2,k3 with
 * dy = k1*g + k2*y + k3  (train: full batch-stat backward; train=0: k1 = gamma*invstd, k2 = k3 = 0) */
int mpn_bn_bwd_finalize(const float* partial, int chunks, int C, int64_t count, const float* gamma, const float* mean,
                        const float* invstd, int train, float* dgamma, float* dbeta, float* coef, void* stream);
/* backward, stage 3: dy = k1*g + k2*y + k3 (k2/k3 may be NULL = 0); dres (optional) receives / accumulates g.  With relu the mask
 * comes from `mask` bits (mpn_bn_act_forward) when given, else from z, else it is recomputed from y (mask_scale / mask_shift). */
int mpn_bn_bwd_apply(const void* dz, const void* z, const void* y, const float* k1, const float* k2, const float* k3,
                     const float* mask_scale, const float* mask_shift, void* dy, void* dres, int dres_accumulate, int64_t P, int C, int Cs, int relu, int dtype,
                     const uint8_t* mask, void* stream);
int mpn_bn_bwd_chunks(int64_t P, int Cs, int dtype);

/* ---------------------------------------------------------------------------------------------
 * Pooling / resampling / layout (fpn.py:84-100, posenet.py:180-184,296-315)
 * -------------------------------------------------------------------------------------------*/
int mpn_maxpool3x3s2_forward(const void* x, void* y, uint8_t* idx, int B, int H, int W, int Cs,
                             int Ho, int Wo, int dtype, void* stream);
int mpn_maxpool3x3s2_backward(const void* dy, const uint8_t* idx, void* dx, int B, int H, int W, int Cs,
                              int Ho, int Wo, int dtype, void* stream);
/* dcoarse[b,h,w,:] (+)= sum over the fine pixels whose nearest source is (h,w) of dfine */
int mpn_upsample_nearest_backward(const void* dfine, void* dcoarse, int B, int Hf, int Wf, int Hc, int Wc,
                                  int Cs, int accumulate, int dtype, void* stream);
/* out[b, oh, ow, c_off + c] = src[b, oh*Hs/Ho, ow*Ws/Wo, c]  (nearest; writes a channel slice) */
int mpn_upsample_nearest_slice(const void* src, void* dst, int B, int Hs, int Ws, int Cs_src,
                               int Ho, int Wo, int Cs_dst, int c_off, int dtype, void* stream);
/* dsrc[b,h,w,c] = sum over fine pixels of ddst[b,oh,ow,c_off+c] */
int mpn_upsample_nearest_slice_backward(const void* ddst, void* dsrc, int B, int Hs, int Ws, int Cs_src,
                                        int Ho, int Wo, int Cs_dst, int c_off, int dtype, void* stream);
/* API edge: padded internal f32/bf16 [B,h,w,Cs] -> exact f32 [B,H,W,C] (nearest up by H/h) and back */
int mpn_export_f32(const void* src, int src_dtype, float* dst, int B, int Hs, int Ws, int Cs, int C,
                   int Ho, int Wo, int64_t dst_sB, int64_t dst_sP, void* stream);
int mpn_import_grad(const float* ddst, int64_t ddst_sB, int64_t ddst_sP, void* dsrc, int dst_dtype,
                    int B, int Hs, int Ws, int Cs, int C, int Ho, int Wo, void* stream);
/* generic strided f32 NCHW -> dense NHWC f32 [B,H,W,C] (ground-truth maps) */
int mpn_nchw_to_nhwc_f32(const float* src, int64_t sB, int64_t sC, int64_t sH, int64_t sW, float* dst,
                         int B, int C, int H, int W, void* stream);
/* detection-head edge: padded internal [B,HW,Cs] <-> dense f32 [B, HW*C] slice of the [B,A,C/9] output
 * (the permute+view+cat of network/posenet.py:67-69,111-117,327-328 without any copy kernels in between) */
int mpn_det_pack(const void* src, int src_dtype, float* dst, int B, int64_t HW, int Cs, int C, int64_t dst_sB, void* stream);
int mpn_det_unpack(const float* ddst, void* dsrc, int dst_dtype, int B, int64_t HW, int Cs, int C, int64_t dst_sB, void* stream);
int mpn_relu_forward(const void* x, void* y, int64_t n, int dtype, void* stream);
int mpn_relu_backward(const void* dz, const void* z, void* dx, int64_t n, int accumulate, int dtype, void* stream);
int mpn_add_inplace(void* dst, const void* src, int64_t n, int dtype, void* stream);
int mpn_channel_sum(const void* dy, int dy_dtype, int64_t P, int C, int Cs, float* partial, int chunks, void* stream);
int mpn_channel_sum_chunks(int64_t P, int Cs, int dtype);
/* db[c] += sum over the P rows of dy[p][c] — small P, any C (Linear-layer bias gradients) */
int mpn_colsum_rows(const void* dy, int dy_dtype, int64_t P, int C, int Cs, float* db, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Losses (posenet.py:367-445, losses.py:5-137)
 * -------------------------------------------------------------------------------------------*/
/* preds: 5 device pointers (f32 NHWC [B,h,w,*] with pixel stride pred_sP[j]); gt/wgt dense NHWC f32
 * [B,h,w,18].  out[0..4] = per-level means, out[5] = total, out[6] = max_ht, out[7] = min_ht. */
int mpn_mse_heatmap_forward(const float* const* preds, const int64_t* pred_sP, const float* gt, const float* wgt,
                            int64_t npix, float* partial, int chunks, float* out, void* stream);
/* dpred_j[p, c] = gscale * 2*w^2*(pred - gt)/N for c < 18, 0 for c in [18, Cj) */
int mpn_mse_heatmap_backward(const float* const* preds, float* const* dpreds, const int64_t* pred_sP,
                             const int64_t* dpred_sP, const int32_t* pred_C, const float* gt, const float* wgt,
                             int64_t npix, const float* gscale, void* stream);
int mpn_mse_chunks(int64_t npix);
/* The two calls above with the person-segmentation term (the K + 1st output channel of the keypoint subnet): mask is the
 * mask_all target, dense f32 [B,h,w] in [0, 1]; pred_C[j] the live channels of prediction j (18 or more).  For every level j
 * with a nineteenth channel (pred_C[j] >= 19)
 *   seg_j = mean over pixels of (pred_j[p, 18] - mask[p])^2 / 100,
 * not weighted by wgt; total = heat-map total + sum_j seg_j.  out f32 [MPN_MSE_SEG_OUT]: [0..7] exactly what
 * mpn_mse_heatmap_forward writes (the same two launches); [8..12] seg_j (0 for a level without the channel); [13] their sum;
 * [14], [15] max / min of channel 18 of the final prediction (0 when it has 18 channels); [16] the total; the rest 0.
 * seg_partial needs seg_chunks * 8 floats, seg_chunks = mpn_mse_seg_chunks(npix).
 * Backward: channels < 18 as mpn_mse_heatmap_backward, bit for bit; dpred_j[p, 18] = gscale * 2 * (pred - mask) / (100 * npix)
 * where pred_C[j] >= 19; channels above 18 are 0.  MPN_E_BADARG before any HIP call: a null or misaligned pointer (dpreds[j] and
 * gscale may be null), npix outside 1..2^31 - 1, a chunk count that is not the function's, pred_C[j] < 18 or above its stride. */
#define MPN_MSE_SEG_OUT 20
int mpn_mse_seg_chunks(int64_t npix);
int mpn_mse_heatmap_seg_forward(const float* const* preds, const int64_t* pred_sP, const int32_t* pred_C, const float* gt,
                                const float* wgt, const float* mask, int64_t npix, float* partial, int chunks, float* seg_partial,
                                int seg_chunks, float* out, void* stream);
int mpn_mse_heatmap_seg_backward(const float* const* preds, float* const* dpreds, const int64_t* pred_sP, const int64_t* dpred_sP,
                                 const int32_t* pred_C, const float* gt, const float* wgt, const float* mask, int64_t npix,
                                 const float* gscale, void* stream);
/* The recorded training step's form of the two calls above (replay.py): loss and gradients in ONE pass over the network's
 * internal tensors, with no exported f32 copies.  levels[0..3] = the intermediate maps k2..k5 (f32, [B, H>>s, W>>s, 32], s = 0..3:
 * posenet.py:243-257 up-samples them by nearest neighbours to the heat-map size, so pixel (y, x) reads level s at (y>>s, x>>s) and
 * a coarse cell's gradient is the sum over its children), levels[4] = the final prediction at [B, H, W, 32]; dlevels[j] receives
 * d(total)/d(levels[j]) in `dtype` with the padding channels zero.  gt / wgt are the reference's NCHW f32 targets read in place
 * (strides g_sB, g_sC, g_sH in elements, unit stride along x).  H and W must be multiples of 8.  out as for
 * mpn_mse_heatmap_forward; partial needs blocks * 8 floats, blocks = mpn_mse_train_blocks(B, H, W).  The gradients are
 * bit-identical to mpn_mse_heatmap_backward + mpn_import_grad. */
int mpn_mse_train_blocks(int B, int H, int W);
int mpn_mse_heatmap_train(const float* const* levels, void* const* dlevels, const int32_t* level_Cs, int dtype,
                          const float* gt, const float* wgt, int64_t g_sB, int64_t g_sC, int64_t g_sH,
                          int B, int H, int W, const float* gscale, float* partial, int blocks, float* out, void* stream);
/* mpn_mse_heatmap_train with the person-segmentation term, for a recorded step with mask_all: the same launch in its seg-aware
 * instantiation.  level_C[j] (18 .. 32) are the live channels of level j; on every level with a nineteenth channel lane 18 is live
 * with w = 1, g = mask (f32 [B][1][H][W] dense, 16-byte aligned, read in place with 16-byte loads) and the scale
 * 2 gscale / (100 B H W); it takes the same 8x8 cell walk, so dlevels[j][.., 18] is bit-identical to
 * mpn_mse_heatmap_seg_backward + mpn_import_grad, and lanes 0..17 to mpn_mse_heatmap_train's.  A level without the channel keeps
 * the zero in lane 18 and is not read there.  out f32 [MPN_MSE_SEG_OUT] as for mpn_mse_heatmap_seg_forward (its two finalize
 * launches); partial needs blocks * 16 floats.  MPN_E_BADARG before any HIP call as for mpn_mse_heatmap_train, and for a null or
 * misaligned mask, level_C outside 18..32, a dtype that is none of the three. */
int mpn_mse_heatmap_seg_train(const float* const* levels, void* const* dlevels, const int32_t* level_Cs, const int32_t* level_C,
                              int dtype, const float* gt, const float* wgt, const float* mask, int64_t g_sB, int64_t g_sC,
                              int64_t g_sH, int B, int H, int W, const float* gscale, float* partial, int blocks, float* out,
                              void* stream);
/* focal + smooth-L1.  cls [B,A] f32 (post-sigmoid), reg [B,A,4], anchors [A,4], anno [B,maxN,5].
 * out[0] = cls loss, out[1] = reg loss (batch means).  per_img [B][4] scratch. */
int mpn_focal_blocks(int A);   /* partial needs B * mpn_focal_blocks(A) * 4 floats */
int mpn_focal_forward(const float* cls, const float* reg, const float* anchors, const float* anno,
                      int B, int A, int maxN, float* partial, float* per_img, float* out, void* stream);
/* gscale: device float[2] = upstream gradients of {cls loss, reg loss} */
int mpn_focal_backward(const float* cls, const float* reg, const float* anchors, const float* anno,
                       int B, int A, int maxN, const float* per_img, const float* gscale,
                       float* dcls, float* dreg, void* stream);
/* the same for K > 1 classes (losses.py:65-77 one-hot targets): cls [B,A,K] f32 (post-sigmoid), dcls [B,A,K] with the same
 * alignment modulo 16 bytes.  A positive anchor is 1 at class int(anno[...,4]) and 0 at the other K - 1; a class id outside [0, K)
 * is never used as an index (such an anchor counts as negative everywhere) and bad[b] (device float[B]) receives the number of
 * valid annotations of image b that carry one.  per_img / out / gscale as above. */
int mpn_focal_mc_blocks(int A);   /* partial needs B * mpn_focal_mc_blocks(A) * 4 floats */
int mpn_focal_forward_mc(const float* cls, const float* reg, const float* anchors, const float* anno, int B, int A, int K,
                         int maxN, float* partial, float* per_img, float* bad, float* out, void* stream);
int mpn_focal_backward_mc(const float* cls, const float* reg, const float* anchors, const float* anno, int B, int A, int K,
                          int maxN, const float* per_img, const float* gscale, float* dcls, float* dreg, void* stream);
/* score[b,a] = max_k cls[b,a,k], cls_id[b,a] = index of the first maximum (torch.max(dim) ties, posenet.py:267,283); K < 4096 */
int mpn_class_max(const float* cls, int B, int A, int K, float* score, int64_t* cls_id, void* stream);
int mpn_sigmoid_forward(const float* x, float* y, int64_t n, void* stream);   /* in place allowed */
/* dlogit = dp * p * (1-p) */
int mpn_sigmoid_backward(const float* dp, const float* p, float* dlogit, int64_t n, void* stream);
/* PRN: out = softmax(relu?(a) + res) rowwise (posenet.py:345-347); BCE mean (posenet.py:436-439) */
int mpn_add_softmax_rows(const float* a, int64_t a_stride, const float* res, float* out, int rows, int cols, int relu, void* stream);
/* dlogit = p*(dp - sum p*dp), masked by pre_relu > 0 when pre_relu != NULL.  a / pre_relu: rows of `cols` values with row
 * stride a_stride / pre_stride (the conv output they come from is padded to a multiple of 32 columns) */
int mpn_softmax_rows_backward(const float* p, const float* dp, const float* pre_relu, int64_t pre_stride, float* dlogit, int rows, int cols, void* stream);
int mpn_bce_mean_backward(const float* p, const float* label, float* dp, int64_t n, const float* gscale, void* stream);
/* nn.Dropout (posenet.py:139,341-342): y = keep(seed, i) ? x / (1 - p) : 0, counter-based (same call with the same seed
 * applied to a gradient is the backward) */
int mpn_dropout(const void* x, void* y, int64_t n, uint64_t seed, float p, int dtype, void* stream);
int mpn_bce_chunks(int64_t n);
int mpn_bce_mean_forward(const float* p, const float* label, int64_t n, float* partial, int chunks, float* out, void* stream);
/* The recorded PRN training step (replay.py).
 * mpn_dropout_dev = mpn_dropout with seed = state[0] + k (wrapping 64-bit), state a device uint64[1] (8-byte aligned): a
 * launch list that holds `state` and `k` draws new masks on every replay.  mpn_dropout_advance: state[0] += inc. */
int mpn_dropout_dev(const void* x, void* y, int64_t n, const uint64_t* state, uint64_t k, float p, int dtype, void* stream);
int mpn_dropout_advance(uint64_t* state, uint64_t inc, void* stream);
/* y[rows][npad] (dtype) = x[rows][n] (f32) rounded to nearest even, columns n .. npad zero: the PRN's input activation */
int mpn_prn_pack(const float* x, void* y, int rows, int n, int npad, int dtype, void* stream);
/* mpn_add_softmax_rows(relu = 1) -> mpn_bce_mean_forward / _backward -> mpn_softmax_rows_backward -> cast, in one launch per
 * row plus the mean finalize: dl[rows][npad] (dtype; columns cols .. npad zero) holds the gradient of mean BCE with respect to
 * the pre-activation o (row stride o_stride), bit-equal to that chain's; loss[0] = mean BCE from `rows` f32 partials (differs
 * from mpn_bce_mean_forward in summation order only).  gscale: device float (NULL = 1).  The probabilities are not stored. */
int mpn_prn_head_train(const float* o, int64_t o_stride, const float* res, const float* label, const float* gscale, void* dl,
                       int rows, int cols, int npad, int dtype, float* partial, float* loss, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Boxes (network/utils.py:19-61, network/posenet.py:266-271)
 * -------------------------------------------------------------------------------------------*/
/* img_w < 0 disables the clip (pure BBoxTransform) */
int mpn_box_decode_clip(const float* anchors, const float* deltas, float* boxes, int B, int A,
                        float img_w, float img_h, void* stream);
/* the same with BBoxTransform's optional coefficients (network/utils.py:8-17): mean_std = {mean[0..3], std[0..3]}, a HOST array */
int mpn_box_decode_clip_ms(const float* anchors, const float* deltas, float* boxes, int B, int A, float img_w,
                           float img_h, const float* mean_std, void* stream);
int mpn_clip_boxes(float* boxes, int64_t n, float img_w, float img_h, void* stream);   /* in place, utils.py:55-59 */
/* compact image-0 candidates with score > thresh into dets[n,5] (x1,y1,x2,y2,score) + src index;
 * order preserved (ascending anchor index).  count[0] receives n. */
int mpn_score_filter(const float* boxes, const float* scores, int A, float thresh, float* dets,
                     int32_t* src_idx, int32_t* count, void* stream);

/* the same for every image of a batch in one launch (BASELINE config 5: batch 64; the reference thresholds image 0 only,
 * posenet.py:271): boxes [B,A,4], scores [B,A]; image b's candidates go to dets[b*A*5 ...] (order preserved),
 * src_idx[b*A ...] (optional), counts[b]. */
int mpn_score_filter_batched(const float* boxes, const float* scores, int B, int A, float thresh, float* dets,
                             int32_t* src_idx, int32_t* counts, void* stream);

/* boxes[k,4], scores[k] = rows keep[0..k) of dets[n,5] */
int mpn_gather_dets(const float* dets, const int64_t* keep, int k, float* boxes, float* scores, void* stream);
/* per image b < B: boxes[b*out_stride*4 ...], scores[b*out_stride ...] = rows keep[b*keep_stride + (0..num[b])) of the
 * image's candidate block dets + b*dets_stride (floats); kmax >= max num[b] sizes the launch */
int mpn_gather_dets_batched(const float* dets, int64_t dets_stride, const int64_t* keep, int64_t keep_stride, const int64_t* num,
                            int B, int kmax, float* boxes, float* scores, int64_t out_stride, void* stream);
/* class ids of the kept detections (posenet.py:283): out[b*out_stride + i] = cls_id[b*A + src[b*A + keep[b*keep_stride + i]]] for
 * i < num[b], 0 for num[b] <= i < kmax; src = the anchor indices mpn_score_filter(_batched) recorded.  num == NULL (B == 1): kmax rows */
int mpn_gather_class(const int64_t* cls_id, const int32_t* src, int A, const int64_t* keep, int64_t keep_stride,
                     const int64_t* num, int B, int kmax, int64_t* out, int64_t out_stride, void* stream);

/* ---------------------------------------------------------------------------------------------
 * NMS — replaces lib/nms: gpu_nms (src/nms_cuda.c:17-67), _nms/nms_kernel
 * (src/cuda/nms_kernel.cu:26-83) and the sort/gather of pth_nms (pth_nms.py:25-44).
 * dets [n,5] f32 device, unsorted.  mode 0: suppress if IoU > thresh (reference GPU path),
 * mode 1: IoU >= thresh (reference CPU path, nms.c:59).  keep_out [n] i64 device receives ORIGINAL
 * indices in descending-score order (ties: lower index first); num_out [1] i64 device.
 * workspace: mpn_nms_workspace_bytes(n) bytes of device memory.
 * -------------------------------------------------------------------------------------------*/
int64_t mpn_nms_workspace_bytes(int64_t n);
int mpn_nms(const float* dets, int64_t n, float thresh, int mode, int64_t* keep_out, int64_t* num_out,
            void* workspace, void* stream);
/* Segmented NMS: B independent problems in the same three launches, sizes read ON THE DEVICE (counts[b] candidates for
 * image b, rows at dets + b*dets_stride floats), so a batch needs no per-image host round trip.  nmax >= max counts[b]
 * sizes the launches and the workspace (mpn_nms_batched_workspace_bytes(B, nmax)); keep_out [B][keep_stride] i64,
 * num_out [B] i64.  Each image's result equals mpn_nms on that image alone. */
int64_t mpn_nms_batched_workspace_bytes(int B, int64_t nmax);
int mpn_nms_batched(const float* dets, int64_t dets_stride, const int32_t* counts, int B, int64_t nmax, float thresh, int mode,
                    int64_t* keep_out, int64_t keep_stride, int64_t* num_out, void* workspace, void* stream);
/* mpn_nms_batched with a cap ahead of the suppression: per image only the top_k best-scored candidates (ties by index: the
 * order of the sort) take part, the rest are dropped.  NOT in the reference (posenet.py:269-285 hands every candidate above
 * 0.05 to nms) and off unless the caller asks: it bounds the N x N/64 mask of a dense image (A = 76 725 at 640x640: 736 MB)
 * to top_k x top_k/64.  workspace: mpn_nms_batched_workspace_bytes(B, min(nmax, top_k)); keep_stride >= min(nmax, top_k). */
int mpn_nms_batched_topk(const float* dets, int64_t dets_stride, const int32_t* counts, int B, int64_t nmax, int64_t top_k,
                         float thresh, int mode, int64_t* keep_out, int64_t keep_stride, int64_t* num_out, void* workspace,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * Class-wise candidates and NMS for a head with K classes.  NOT in the reference, whose post-processing takes the maximum over
 * the classes ahead of the threshold (posenet.py:267-271: one candidate per anchor, suppression across classes) — this is the
 * form a RetinaNet is scored with, and opt-in (ops.detect_batched_classwise).  boxes [B,A,4] f32 (16-byte aligned), cls [B,A,K]
 * f32 (any 4-byte aligned address: an image's base is not 16-byte aligned when A*K % 4 != 0), A*K < 2^31.
 *   candidates   every flat index f = a*K + c with cls[b,a,c] > thresh (strict: a NaN or a score equal to thresh does not pass),
 *                in ascending f; row (boxes[b,a], cls[b,a,c]), class c = f % K, anchor a = f / K
 *   suppression  in descending score, ties lower f first; a kept candidate suppresses a later one iff both have the SAME class
 *                and devIoU (nms_kernel.cu:16-24) > thresh (mode 0) / >= thresh (mode 1); top_k as mpn_nms_batched_topk: the
 *                top_k best-scored candidates of the IMAGE (not of each class), ties lower f first, 0 = all of them
 *   output       keep_out: rows of the candidate list in descending score across classes, ties lower f first
 * With K == 1 every list equals mpn_score_filter_batched + mpn_nms_batched(_topk) byte for byte.
 * Two passes over cls (the outputs are sized from the counted totals, never A*K rows), grid = (chunks, B) with
 * mpn_class_filter_chunk() flat indices per chunk; positions come from bit counts, wave scans and the chunk table, never from
 * atomics: the same bytes on every launch and at every position in the batch.
 *   mpn_class_filter_count  chunk_cnt [B][chunks] i32 (mpn_class_filter_workspace_bytes(B, A, K) bytes; chunks =
 *                           ceil(A*K / mpn_class_filter_chunk())) and counts [B] i32 = candidates per image
 *   mpn_class_filter_fill   from the SAME cls, thresh and chunk_cnt: dets [B][dets_stride] f32 (rows of 5; dets_stride >= nmax*5),
 *                           cand_cls / cand_anchor [B][idx_stride] i32 (idx_stride >= nmax), counts [B] = min(candidates, nmax);
 *                           nmax >= max counts[b] of the count pass (rows at and beyond nmax are never written)
 *   mpn_nms_batched_classes mpn_nms_batched(_topk) with cand_cls[b*cls_stride + i] the class of row i (cls_stride >= nmax): the
 *                           same kernels, nms_rank_kernel<true> / nms_mask_kernel<true> in place of the <false> instantiations;
 *                           workspace mpn_nms_batched_classes_workspace_bytes(B, top_k > 0 ? min(nmax, top_k) : nmax): the layout
 *                           of mpn_nms_batched plus the sorted classes; keep_stride >= that row count
 *   mpn_gather_cand_class   classes[b*out_stride + i] = cand_cls[b*idx_stride + keep[b*keep_stride + i]] as int64 for i < num[b],
 *                           0 for num[b] <= i < kmax (mpn_gather_class's padding); anchors (optional, with cand_anchor) the same.
 *                           Boxes and scores: mpn_gather_dets_batched.
 * -------------------------------------------------------------------------------------------*/
int mpn_class_filter_chunk(void);
int64_t mpn_class_filter_workspace_bytes(int B, int A, int K);   /* MPN_E_BADARG for B, A, K <= 0 or A*K >= 2^31 */
int mpn_class_filter_count(const float* cls, int B, int A, int K, float thresh, int32_t* chunk_cnt, int32_t* counts, void* stream);
int mpn_class_filter_fill(const float* boxes, const float* cls, int B, int A, int K, float thresh, const int32_t* chunk_cnt,
                          int64_t nmax, float* dets, int64_t dets_stride, int32_t* cand_cls, int32_t* cand_anchor,
                          int64_t idx_stride, int32_t* counts, void* stream);
int64_t mpn_nms_batched_classes_workspace_bytes(int B, int64_t nmax);
int mpn_nms_batched_classes(const float* dets, int64_t dets_stride, const int32_t* cand_cls, int64_t cls_stride,
                            const int32_t* counts, int B, int64_t nmax, int64_t top_k, float thresh, int mode, int64_t* keep_out,
                            int64_t keep_stride, int64_t* num_out, void* workspace, void* stream);
int mpn_gather_cand_class(const int32_t* cand_cls, const int32_t* cand_anchor, int64_t idx_stride, const int64_t* keep,
                          int64_t keep_stride, const int64_t* num, int B, int kmax, int64_t* classes, int64_t* anchors,
                          int64_t out_stride, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Optimizer: torch.optim.Adam semantics (training/multipose_keypoint_train.py:106-110), fused over
 * a flat f32 arena.  step_size/bias corrections are computed on the host and passed in.
 * -------------------------------------------------------------------------------------------*/
int mpn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float lr, float beta1, float beta2, float eps, float weight_decay,
                  float bias_correction1, float bias_correction2_sqrt, float grad_scale, void* stream);
/* The same update with every scalar read from DEVICE memory, so that a captured hipGraph of the training step replays
 * correct Adam steps: hyper[0..7] = {lr, beta1, beta2, eps, weight_decay, grad_scale, bias_correction1,
 * sqrt(bias_correction2)} (floats), hyper[8] = step count (int32 bits).  mpn_adam_advance does step += 1 and recomputes
 * hyper[6..7] (double-precision pow of the FLOAT betas in hyper[1..2]: Adam with the float32-rounded betas, within 2.4e-7 /
 * 6.5e-6 relative of the values torch forms from the host doubles, see weight_prep.hip); mpn_adam_step_dev applies one update to a
 * 16-byte aligned run of the arena.  The host only rewrites hyper[0] when the scheduler changes the learning rate. */
int mpn_adam_advance(float* hyper, void* stream);
int mpn_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* hyper,
                      void* stream);
/* Gradient clipping by the infinity norm (the reference Trainer's max_grad_norm: torch.nn.utils.clip_grad_norm_(params, max_norm,
 * inf)), every scalar on the device.  mpn_grad_absmax_partial reduces max |g| over one 16-byte aligned run of n floats to
 * mpn_grad_absmax_workspace_bytes(n) / 4 partials (one launch per run, each into its own consecutive slots; a NaN anywhere gives a
 * NaN).  mpn_grad_clip_finalize reduces nparts partials and writes *total = max (the norm torch returns) and
 * *coef = min(reciprocal(total + 1e-6f) * *max_norm, 1) (NaN stays NaN), max_norm read from device memory.
 * mpn_scale_by_dev does x *= *s over a 16-byte aligned run (torch scales p.grad in place); mpn_adam_step_clip_dev is
 * mpn_scale_by_dev(grad, n, coef) followed by mpn_adam_step_dev: the update of torch's clip followed by step(), bit for bit. */
int64_t mpn_grad_absmax_workspace_bytes(int64_t n);
int mpn_grad_absmax_partial(const float* grad, int64_t n, float* partials, void* stream);
int mpn_grad_clip_finalize(const float* partials, int64_t nparts, const float* max_norm, float* total, float* coef, void* stream);
int mpn_adam_step_clip_dev(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* hyper,
                           const float* coef, void* stream);
int mpn_scale_by_dev(float* x, int64_t n, const float* s, void* stream);
int mpn_fill_f32(float* dst, float v, int64_t n, void* stream);
/* device-to-device copy on the stream (gradient hand-over between two activations of equal geometry) */
int mpn_copy_bytes(void* dst, const void* src, int64_t nbytes, void* stream);
/* log vector of a recorded training step (replay.py): kp8 = out of mpn_mse_heatmap_forward (or NULL), det2 = out of
 * mpn_focal_forward (or NULL); logv[0..7] = kp8, [8] = cls + reg, [9] = cls, [10] = reg, [11] = loss (the sums the reference
 * forms with torch adds at posenet.py:387,421 and the combined step of SURVEY.md 8d) */
int mpn_step_log(const float* kp8, const float* det2, float* logv, void* stream);
/* mpn_step_log for a step with the person-segmentation term: kp is the MPN_MSE_SEG_OUT vector of mpn_mse_heatmap_seg_forward
 * (required), logv f32 [MPN_STEP_LOG_SEG]: [0..12] keep mpn_step_log's meaning with [11] = kp[16] + the detection total ([12] is the
 * gradient clip's), [13..17] the seg means, [18] their sum, [19] / [20] max / min of channel 18 of the final prediction. */
#define MPN_STEP_LOG_SEG 21
int mpn_step_log_seg(const float* kp, const float* det2, float* logv, void* stream);

/* ---------------------------------------------------------------------------------------------
 * conv2 of the keypoint head by position classes (network/posenet.py:311-315: conv2 over cat(up8(q5), up4(q4), up2(q3), q2)).
 * The x8 / x4 members contribute through nine class maps each at their own resolution (csrc/conv2cls.hip has the derivation);
 * these entry points are the streaming pieces around the ordinary convolution launches.  O = output channels (256), C = channels
 * per member (128); w / dw: f32 [O][3][3][4 C].
 *   comb (f32, mpn_conv2cls_comb_elems(O, C) elements) = Wm [O][3][3][2C] | Wc8 [9 O][3][3][C] | Wc4 [9 O][3][3][C] (frame filters of
 *          the forward class convolutions) | Wtap8 [9 O][C] | Wtap4 [9 O][C] (row t * O + o = tap t of output channel o)
 *   combine: comb <- w;      fold: dw += dcomb, dcomb = dWm [O][3][3][2C] | dWtap8 [9 O][C] | dWtap4 [9 O][C]
 *   tapsum : g[b,i,j,t*O+:] ([B,h,w,9 O] in `dtype`) = sum of dy over the output pixels whose tap t reads (i, j), from the class sums pc
 *            of the member up-sampled by s (8 or 4)
 *   expand : e[b,y,x,:] ([B,H,W,O] in `dtype`) = m8[b, y/8, x/8, class * O + :] + m4[b, y/4, x/4, class * O + :]   (m: f32 [B,h,w,9 O])
 *   classsum: m (f32 class maps) from t (f32 [B,h,w,9 O], t[..., tap * O + :] = the 1x1 convolution with filter tap `tap`): the forward
 *            per tap, used where the zero taps of the frame filters cost matrix time (f32)
 *   pool   : p8 / p4 ([B,H/s,W/s,9 O] in `dtype`) = per-class sums of dy ([B,H,W,O]) over s x s blocks; H, W multiples of 8
 * MPN_F16 backward (unweighted sums of up to 64 dy pass fp16's range long before dy does): pool writes p8 / p4 in F32 and tapsum
 * reads them so; tapsum stores g / s^2; the 1x1 input-gradient launch over g gives the s^2 back through MpnConvParams.scale, and fold
 * (`dtype`: the type of that backward) multiplies the dWtap8 / dWtap4 slices of dcomb (contracted with g / s^2) by 64 / 16.  In
 * MPN_BF16 / MPN_F32 p is stored in `dtype` and nothing is scaled.
 * -------------------------------------------------------------------------------------------*/
int64_t mpn_conv2cls_comb_elems(int O, int C);
int mpn_conv2cls_combine(const float* w, float* comb, int O, int C, void* stream);
int mpn_conv2cls_expand(const float* m8, const float* m4, void* e, int B, int H, int W, int O, int dtype, void* stream);
int mpn_conv2cls_classsum(const float* t, float* m, int B, int h, int w, int O, void* stream);
int mpn_conv2cls_pool(const void* dy, void* p8, void* p4, int B, int H, int W, int O, int dtype, void* stream);
int mpn_conv2cls_tapsum(const void* pc, void* g, int B, int h, int w, int O, int s, int dtype, void* stream);
int mpn_conv2cls_fold(const float* dcomb, float* dw, int O, int C, int dtype, void* stream);

/* library self-description */
const char* mpn_version(void);

/* ---------------------------------------------------------------------------------------------
 * Training augmentation from raw uint8 sources (datasets/coco_data/ImageAugmentation.py:25-231 aug_scale, aug_rotate,
 * aug_croppad, aug_flip; COCO_data_pipeline.py:211-215; preprocessing.py:15-26), one launch per batch, one cubic
 * (A = -0.75) sample per output element through the composed inverse transform, taps clamped to the source, no
 * intermediate image and no uint8 rounding.  Coordinates are float64, weights and the 16-term sum float32.
 *
 * src: the packed sources of the whole batch (device, src_bytes long).  table: double [B][MPN_AUG_COLS] (device), per
 * sample: byte offset and row pitch of its BGR image ([H][W][3]) and of its mask ([H][W]) in their packed buffers,
 * H, W, the resize factor, the scaled size (nw, nh), the rotated canvas size (cw, ch), the row-major 2x3 INVERSE of
 * the matrix handed to warpAffine, the canvas pixel (ox, oy) of crop pixel (0, 0), and the flip flag.  A row whose
 * source does not lie inside [0, src_bytes) is not dereferenced: its outputs are NaN.
 *
 * mpn_augment_image: out f32 [B][3][crop_y][crop_x], plane c = (BGR[2 - c] / 255 - mean[c]) / std[c] with
 *   mean_std = {mean[3], std[3]} (HOST pointer, RGB order); outside the canvas or the scaled image the BGR value is 128.
 * mpn_augment_mask: out f32 [B][18][gh][gw]; cell (i, j) samples the (crop_x + 1)-wide mask crop at
 *   ((j + 0.5) stride - 0.5, (i + 0.5) stride - 0.5), flipped over that width; border value 255; result / 255 written
 *   to all 18 channels.
 * -------------------------------------------------------------------------------------------*/
#define MPN_AUG_IMG_OFF 0
#define MPN_AUG_IMG_PITCH 1
#define MPN_AUG_MASK_OFF 2
#define MPN_AUG_MASK_PITCH 3
#define MPN_AUG_H 4
#define MPN_AUG_W 5
#define MPN_AUG_SCALE 6
#define MPN_AUG_NW 7
#define MPN_AUG_NH 8
#define MPN_AUG_CW 9
#define MPN_AUG_CH 10
#define MPN_AUG_MINV 11
#define MPN_AUG_OX 17
#define MPN_AUG_OY 18
#define MPN_AUG_FLIP 19
#define MPN_AUG_COLS 20
int mpn_augment_image(const uint8_t* src, int64_t src_bytes, const double* table, int B, float* out, int crop_y, int crop_x,
                      const float* mean_std, void* stream);
int mpn_augment_mask(const uint8_t* src, int64_t src_bytes, const double* table, int B, float* out, int gh, int gw, int stride,
                     int crop_x, void* stream);
/* mpn_augment_plane: mpn_augment_mask's sampling (the same table row with its MASK columns, the same mapping, the same single
 *   4x4 cubic sample, clamp and / 255) of ANY uint8 plane, with an explicit value outside the canvas or the scaled image
 *   (`outside`, in 0 .. 255, divided by 255 like a sample) and ONE output channel: out f32 [B][1][gh][gw].  For mask_all the
 *   outside value is 0: nobody stands outside the image.                                                                    */
int mpn_augment_plane(const uint8_t* src, int64_t src_bytes, const double* table, int B, float* out, int gh, int gw, int stride,
                      int crop_x, float outside, void* stream);

/* Boxes of the instance masks of a detection batch (ImageAugmentation.py:234-340 aug_*_bbox on the masks,
 * COCO_data_pipeline.py:382-405 get_ground_truth, :444-458 bbox_collater) without any warped mask.
 *
 * table: double [n_inst][MPN_AUGB_COLS] (device), one row per non-crowd instance: columns 0 .. MPN_AUG_COLS - 1 are the
 * row of the instance's SAMPLE (H, W = the full source size; the IMG columns are not read), except that MASK_OFF /
 * MASK_PITCH address the instance's own bounding rectangle in the packed buffer src (uint8, non-zero = 1, src_bytes
 * long); columns MPN_AUGB_RX0 .. RH place that rectangle in the H x W source (0 <= rx0, rx0 + rw <= W, rw >= 1; same
 * for y).  Outside the rectangle the mask is 0 by construction, so a tap there reads 0 and is not dereferenced.
 *
 * Scan launch (grid z = instance): pixel (u, v) of the (crop_y + 1) x (crop_x + 1) mask frame is un-flipped over crop_x
 * (u -> crop_x - u), moved by (ox, oy), mapped and sampled as mpn_augment_mask does (float64 coordinates, float32 cubic
 * weights, the same accumulation order); it is ON when the sum is >= 0.5f; outside the canvas or the scaled image it is
 * OFF.  Per (instance, tile of 64 x 16 pixels) one int32 record {min x, max x, min y, max y, flag} goes to workspace
 * (mpn_augment_boxes_workspace_bytes(n_inst, crop_y, crop_x) bytes, device, caller-owned, no initialisation needed).
 * Finalize launch (one wave per output row): row_inst int32 [n_rows] (device) names the instance of output row
 * b * N + r or -1; out f32 [n_rows][5] = {x1, y1, x2 + 1, y2 + 1, 0} over the ON pixels, five -1 for an instance
 * with no ON pixel and for a -1 row, five NaN for an instance whose rectangle does not lie inside its source or
 * inside [0, src_bytes) (never dereferenced) and for a row_inst entry >= n_inst.  n_inst == 0 and n_rows == 0 are
 * allowed (the launch is skipped).  Nothing is allocated or synchronised.
 */
#define MPN_AUGB_RX0 20
#define MPN_AUGB_RY0 21
#define MPN_AUGB_RW 22
#define MPN_AUGB_RH 23
#define MPN_AUGB_COLS 24
int64_t mpn_augment_boxes_workspace_bytes(int n_inst, int crop_y, int crop_x);
int mpn_augment_boxes(const uint8_t* src, int64_t src_bytes, const double* table, int n_inst, const int32_t* row_inst, int n_rows,
                      float* out, int crop_y, int crop_x, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * COCO segmentations rasterised on the device (csrc/segm.hip; datasets/segm.py packs the tables): annToMask by the rule of
 * maskApi.c (rleFrPoly on the 5x grid, union of an annotation's parts, rleDecode), byte for byte.
 *
 * insts: int64 [n_inst][MPN_SEGI_COLS] (device): the image's H, W; a rectangle (rx0, ry0, rw, rh) inside it that contains every
 *   ON cell of the instance (it need not be tight); byte offset and row pitch of that rectangle's row-major uint8 output in
 *   `out`; the instance's parts [p0, p1).
 * parts: int64 [n_parts][MPN_SEGP_COLS] (device): the part's instance; its vertices [v0, v1) (none for an RLE, which is one
 *   part); the offset, in 64-bit words, of its toggle bitmap in the workspace: (H / 64 + 1) * rw words, word k of rectangle column
 *   c at [k * rw + c], slot yd of a column (0 .. H) is bit yd % 64 of word yd / 64.
 * verts: int32 [n_verts][2], the vertices (int)(5 x + 0.5), (int)(5 y + 0.5); edge e runs from vertex e to vertex e + 1, the
 *   last edge of a part back to v0.  vpart: int32 [n_verts], the part of each.  estart: int32 [n_verts + 1], estart[0] = 0,
 *   estart[e + 1] - estart[e] = max(|dX|, |dY|) of edge e; n_steps = estart[n_verts].
 * toggles: int32 [n_tog][2] = (part, flat column-major index x * H + y) of the RLE parts: the cumulative sums of the run lengths.
 *
 * Launches: memset of the workspace (ws_bytes >= mpn_segm_workspace_bytes(total bitmap words)) and of any_on; one lane per
 * (edge, step) and one per listed toggle flip one bit each (atomic XOR on a word: order-independent, pairs cancel); the fill
 * launch (grid: 64-column tiles up to max_rw, 512-row tiles up to max_h, instances) takes the prefix parity along the flat index
 * of every part, ORs the parts and stores the rectangle; any_on int32 [n_inst] = 1 where an instance has an ON cell, else 0.
 * dense = 1 zeroes all out_bytes of `out` first (rectangles inside [n][H][W] planes); dense = 0 writes the rectangles only.
 * A table row that names something outside its table, its image or its buffer is skipped, never dereferenced.
 * MPN_E_BADARG before any HIP call: null or misaligned pointer, n_inst outside 1..65535, a negative count, n_steps >= 2^31 or > 0
 * without vertices, max_rw / max_h outside 1..65536, out_bytes outside 1..2^40, ws_bytes < 8 or no multiple of 8, dense not 0 / 1.
 * mpn_segm_workspace_bytes: 8 * max(words, 1); 0 for words < 0 or >= 2^31.  Nothing is allocated or synchronised.
 * -------------------------------------------------------------------------------------------*/
#define MPN_SEGI_H 0
#define MPN_SEGI_W 1
#define MPN_SEGI_RX0 2
#define MPN_SEGI_RY0 3
#define MPN_SEGI_RW 4
#define MPN_SEGI_RH 5
#define MPN_SEGI_OUT_OFF 6
#define MPN_SEGI_OUT_PITCH 7
#define MPN_SEGI_P0 8
#define MPN_SEGI_P1 9
#define MPN_SEGI_COLS 10
#define MPN_SEGP_INST 0
#define MPN_SEGP_V0 1
#define MPN_SEGP_V1 2
#define MPN_SEGP_BM 3
#define MPN_SEGP_COLS 4
int64_t mpn_segm_workspace_bytes(int64_t words);
int mpn_segm_rasterize(const int64_t* insts, int n_inst, const int64_t* parts, int n_parts, const int32_t* verts,
                       const int32_t* vpart, const int32_t* estart, int n_verts, int64_t n_steps, const int32_t* toggles,
                       int n_tog, int max_rw, int max_h, uint8_t* out, int64_t out_bytes, int dense, int32_t* any_on,
                       void* workspace, int64_t ws_bytes, void* stream);

/* mask_miss of n_img images from their person annotations (what the reference reads as the mask_miss PNGs under mask2014,
 * datasets/coco_data/COCO_data_pipeline.py:244-250), composed on the device without any instance mask in memory.
 *
 * insts, parts, verts, vpart, estart, toggles, workspace: as for mpn_segm_rasterize (its toggle launches run unchanged); the OUT
 *   columns of insts are not used.  n_inst may be 0 (no image has an annotation to rasterise): insts, kind, parts may then be null.
 * kind: int32 [n_inst], MPN_SEGK_KEYPOINTS / _NO_KEYPOINTS / _CROWD.
 * imgs: int64 [n_img][MPN_SEGM_COLS] (device): the image's H, W; its instances [i0, i1) in annotation order (each with this H, W);
 *   byte offset and row pitch of its H x W uint8 plane in `out`.
 * Rule, with M the annToMask of an instance, walking an image's instances in order from all = miss = 0:
 *   KEYPOINTS: all |= M;   NO_KEYPOINTS: all |= M, miss |= M;   CROWD: miss |= M & ~all (all as accumulated so far);
 *   plane = 255 where miss == 0, else 0.  An image without instances is all 255.
 * Launches: the workspace memset and the toggle launches, then one compose launch (grid: 64-column tiles up to max_w, 512-row
 * tiles up to max_h, images).  No atomics in the compose launch; every byte of every plane is written, nothing between planes.
 * A table row that names something outside its table, its image or its buffer is skipped, never dereferenced.
 * MPN_E_BADARG before any HIP call: null or misaligned pointer, n_img outside 1..65535, n_inst outside 0..65535, a negative count,
 * n_steps >= 2^31 or > 0 without vertices, max_w / max_h outside 1..65536, out_bytes outside 1..2^40, ws_bytes < 8 or no multiple
 * of 8.  Nothing is allocated or synchronised.                                                                                  */
#define MPN_SEGK_KEYPOINTS 0
#define MPN_SEGK_NO_KEYPOINTS 1
#define MPN_SEGK_CROWD 2
#define MPN_SEGM_H 0
#define MPN_SEGM_W 1
#define MPN_SEGM_I0 2
#define MPN_SEGM_I1 3
#define MPN_SEGM_OUT_OFF 4
#define MPN_SEGM_OUT_PITCH 5
#define MPN_SEGM_COLS 6
int mpn_segm_mask_miss(const int64_t* imgs, int n_img, const int64_t* insts, const int32_t* kind, int n_inst, const int64_t* parts,
                       int n_parts, const int32_t* verts, const int32_t* vpart, const int32_t* estart, int n_verts, int64_t n_steps,
                       const int32_t* toggles, int n_tog, int max_w, int max_h, uint8_t* out, int64_t out_bytes, void* workspace,
                       int64_t ws_bytes, void* stream);

/* mask_miss AND mask_all of n_img images from the same tables, toggle launches and ONE compose launch (the compose kernel's
 * second instantiation).  mask_all is the target of the keypoint subnet's person-segmentation channel: 255 where ANY of the
 * image's person annotations covers the pixel (KEYPOINTS, NO_KEYPOINTS and CROWD alike: a plain union, independent of the
 * order), else 0; an image without instances is all 0.  Every listed instance counts, so the caller must not drop the
 * KEYPOINTS instances that cannot change mask_miss.
 * out_miss, out_all: two buffers of out_bytes each; image b's planes lie at the SAME MPN_SEGM_OUT_OFF / MPN_SEGM_OUT_PITCH of
 *   both, validated alike.  out_miss holds the bytes mpn_segm_mask_miss writes for the same arguments.
 * MPN_E_BADARG before any HIP call: as for mpn_segm_mask_miss, and out_all null or closer than out_bytes to out_miss.                       */
int mpn_segm_person_masks(const int64_t* imgs, int n_img, const int64_t* insts, const int32_t* kind, int n_inst, const int64_t* parts,
                          int n_parts, const int32_t* verts, const int32_t* vpart, const int32_t* estart, int n_verts, int64_t n_steps,
                          const int32_t* toggles, int n_tog, int max_w, int max_h, uint8_t* out_miss, uint8_t* out_all,
                          int64_t out_bytes, void* workspace, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PRN training pairs from raw COCO annotations (datasets/coco_data/prn_data_pipeline.py:33-111), one launch per batch.
 * Per sample b: box[b] = the annotation's raw (x, y, w, h); own_kp[b] = its 17 (x, y, v) keypoints; the annotations of its image
 * (the own one, crowds and people with few keypoints among them), in the image's annotation order, are rows
 * person_off[b] .. person_off[b + 1] of img_kp [P][17][3] (offsets outside 0..P are clamped on the device: img_kp is never read
 * out of range).  H = 28 coeff, W = 18 coeff, coeff 1..3.  Both results are f32 [B][H][W][17], channel c = COCO joint
 * (0, 6, 8, 10, 5, 7, 9, 12, 14, 16, 11, 13, 15, 2, 1, 4, 3)[c]:
 *   input = the reference's `weights`: every v > 0 keypoint of the image's annotations that passes the margin test on the raw box
 *           floats (:85-86) sets its cell through the one-branch clamp chain (:90-103), blurred with taps9 ('nearest');
 *   label = the reference's `output`: the own v > 0 keypoints, no margin test, the chain of :56-72 with its try/except, blurred
 *           with taps17 ('constant', 0).
 * Cell arithmetic in float64 with int() truncation and Python's negative-index wrap; blur along axis 0 then axis 1 in
 * scipy.ndimage.correlate1d's summation order with the caller's float64 taps (scipy's _gaussian_kernel1d for sigma 1 radius 4 and
 * sigma 2 radius 8); one rounding to f32.  err[b] (written for every b, with vector stores) is 0 or an OR of MPN_PRN_ERR_* where
 * the reference raises; both maps of such a sample are zero.  All pointers are device pointers; doubles 8-byte aligned.
 * -------------------------------------------------------------------------------------------*/
#define MPN_PRN_ERR_INDEX 1      /* IndexError: x0 >= W with y0 < -H, or (input only) y0 >= H with x0 < -W */
#define MPN_PRN_ERR_ZERODIV 2    /* ZeroDivisionError: ceil(w) == 0 or ceil(h) == 0 */
#define MPN_PRN_ERR_NONFINITE 4  /* ValueError / OverflowError of int() or math.ceil on a NaN or an infinity */
int mpn_prn_train_maps(const double* box, const double* own_kp, const double* img_kp, const int32_t* person_off, int B, int P,
                       int coeff, double threshold, const double* taps9, const double* taps17, float* input, float* label,
                       int32_t* err, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ground-truth heat-maps (datasets/coco_data/heatmap.py:20-41 + COCO_data_pipeline.py:218-236,283):
 * out[b][k][y][x] (f32, 18 keypoint channels) = min(1, sum over people j < num_people[b] with
 * visibility <= 1 of exp(-e) where e = d2/2/sigma/sigma <= 4.6052), float64 arithmetic in annotation
 * order.  joints: double [B][maxP][18][3] = (x, y, visibility) in crop pixels.
 * -------------------------------------------------------------------------------------------*/
int mpn_gt_heatmaps(const double* joints, const int32_t* num_people, int B, int maxP, float* out, int gh, int gw,
                    double stride, double sigma, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Heat-map peak extraction (network/joint_utils.py:19-31 find_peaks, :61-138 NMS).  heat: f32, element
 * (b, j, y, x) at heat[b*sB + j*sJ + y*sY + x*sX].  A cell is a peak if it is > thre1 and no 4-neighbour
 * is larger.  peaks[b][j][slot][4] = (x, y, score, id) as doubles, slots in row-major cell order, ids
 * counted over joints 0..J-1 in that order; with refine != 0 the position/score come from the bicubically
 * (cv2 INTER_CUBIC) `upsamp`-times up-sampled 5x5 patch around the cell, else from the cell itself
 * ((c + 0.5)*upsamp - 0.5, rounded half to even).  counts[b][j] = number of peaks found (only the first
 * `cap` are stored).  workspace: mpn_heatmap_peaks_workspace_bytes(B, J, H, W, cap) bytes of device scratch (one flag bit
 * per cell, the device-wide peak list of the refinement launch); contents need no initialisation.  Three launches: flags
 * (coalesced in channels-last [sJ == 1, sX == J] and planar [sX == 1] layouts), per-plane compaction, refinement.
 * -------------------------------------------------------------------------------------------*/
int64_t mpn_heatmap_peaks_workspace_bytes(int B, int J, int H, int W, int cap);
int mpn_heatmap_peaks(const float* heat, int64_t sB, int64_t sJ, int64_t sY, int64_t sX, int B, int J, int H, int W,
                      float thre1, double upsamp, int refine, double* peaks, int32_t* counts, int cap, void* workspace,
                      void* stream);

/* mpn_heatmap_peaks with the reference's bool_gaussian_filt=True (joint_utils.py:115-116): the up-sampled float32 patch of every peak
 * goes through scipy.ndimage.gaussian_filter before the arg-max, and the score is the SMOOTHED value at the first row-major maximum.
 * taps: HOST pointer to the 2*radius + 1 float64 weights (scipy's _gaussian_kernel1d; sigma 3 -> radius 12, 25 weights); they are
 * copied into the launch.  The smoothing, restated op for op:
 *   - axis 0 (columns) first, then axis 1 (rows); each pass works line by line on values widened to float64;
 *   - a line of n values is extended by `radius` at both ends with scipy's 'reflect' rule applied periodically: index i maps to
 *     m = i mod 2n (non-negative), and m >= n maps to 2n - 1 - m — with n <= radius the extension wraps more than once;
 *   - output l is  t = x[l]*w[radius];  then for k = radius, ..., 1:  t += (x[l-k] + x[l+k]) * w[radius-k]  in exactly this order,
 *     float64, no contraction;
 *   - one rounding to float32 at the end of each pass (the array between the passes is float32).
 * Same workspace (mpn_heatmap_peaks_workspace_bytes), same flags and compaction launches; the third launch is the smoothed refinement
 * kernel (one workgroup per peak, both planes in LDS).  With refine == 0 the taps are validated and the call is mpn_heatmap_peaks.
 * MPN_E_BADARG before any HIP call for a null taps pointer, radius < 1 or > 16, or taps that are not bitwise symmetric;
 * MPN_E_UNSUPPORTED when refine != 0 and rint(5 * upsamp) > 64 (the widest patch the LDS planes hold). */
int mpn_heatmap_peaks_smooth(const float* heat, int64_t sB, int64_t sJ, int64_t sY, int64_t sX, int B, int J, int H, int W,
                             float thre1, double upsamp, int refine, const double* taps, int radius, double* peaks,
                             int32_t* counts, int cap, void* workspace, void* stream);

/* cv2.resize for float32 images / heat-map stacks (evaluate/tester.py:67,213,296-299): src element (y, x, c) at
 * src[y*sY + x*sX + c*sC]; dst dense [Hd][Wd][C]; cubic != 0 -> INTER_CUBIC, else INTER_LINEAR (OpenCV's coordinate rule
 * (d + 0.5)*scale - 0.5, clamped taps, horizontal then vertical pass, float32).  scale = src/dst (the dsize call form) unless
 * inv_fy / inv_fx > 0: those are 1/fy, 1/fx of the `cv2.resize(img, None, fx=, fy=)` form (tester.py:68), used as the scale exactly. */
int mpn_resize(const float* src, int64_t sY, int64_t sX, int64_t sC, int Hs, int Ws, int C, float* dst, int Hd, int Wd,
               int cubic, double inv_fy, double inv_fx, void* stream);

/* Multi-scale + flip test-time augmentation (evaluate/tester.py:143-175,256-331), the element-wise ends around the network.
 *
 * mpn_tta_input: the network input of ONE scale for the pair {image, horizontally mirrored image} in one launch.  img: the decoded
 * float32 image, element (y, x, c) at img[y*sY + x*sX + c*sC], [H][W][3] BGR 0..255.  out: dense float32 [2][3][hp][wp]; image 0 is
 * the original, image 1 the mirrored one (it reads source column W - 1 - x; no mirrored copy exists).  Per image exactly
 * crop_with_factor + resnet_preprocess: INTER_LINEAR resize to (h, w) in the fx/fy form with inv_scale = 1/f as the scale on both
 * axes and mpn_resize's clamp rules, the value 128 from (h, w) up to (hp, wp), then BGR -> RGB, times the float32 reciprocal of 255
 * (how the tensor library divides a float32 tensor by a host scalar), minus mean, correctly rounded division by std, channel-planar.
 * MPN_E_BADARG before any HIP call for null pointers, non-positive sizes or scale, h > hp or w > wp. */
int mpn_tta_input(const float* img, int64_t sY, int64_t sX, int64_t sC, int H, int W, float* out, int h, int w, int hp, int wp,
                  double inv_scale, void* stream);

/* One scale of mpn_tta_merge: the x4-upsampled, cropped pair map, float32, element (y, x, ch) at u[y*pitch + x*36 + ch] for
 * y < rh, x < rw; channels 0..17 from the pass over the original image, 18..35 from the pass over the mirrored one. */
typedef struct MpnTtaScale {
    const float* u;
    int32_t rh, rw;
    int64_t pitch;           /* floats between rows, >= 36 * rw */
} MpnTtaScale;

/* mpn_tta_merge: the averaged maps of an image from the pair maps of its n_scales (1..8) scales in one launch.  scales: HOST table
 * (copied into the launch); swap: HOST pointer to the 18-entry left/right channel permutation (validated, copied into the launch);
 * out: dense float32 [H][W][18].  With R(U, y, x, ch) the INTER_CUBIC sample of U[:rh, :rw, ch] at destination (y, x) of an (H, W)
 * grid in the dsize form, computed as mpn_resize computes it, and r = (float)(1.0 / n_scales):
 *   a_o = sum over the table, in order, of (double)(R(U_s, y, x, c) * r)                      (float32 product, float64 sum)
 *   a_f = sum over the table, in order, of (double)(R(U_s, y, W - 1 - x, 18 + swap[c]) * r)
 *   out[y][x][c] = (float)((a_o + a_f) / 2)
 * — _get_outputs for both images, _handle_heat and the final .float() with their rounding points.
 * MPN_E_BADARG before any HIP call for null pointers, n_scales outside 1..8, a non-positive size, a pitch below 36 * rw or a swap
 * table that is not a permutation of 0..17. */
int mpn_tta_merge(const MpnTtaScale* scales, int n_scales, const int32_t* swap, float* out, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Person masks at inference: channel 18 of a person_seg model's maps -> an image-sized binary mask, and its score against
 * mask_all (csrc/seg_infer.hip; evaluate/tester.py: return_masks, Tester.seg_eval).  The reference never ran this channel, so the
 * definitions are this project's own; they are the op sequences the unfused Tester paths use for channels 0..17.
 *
 * q is channel 18 of the exported float32 maps of one image, thr a float32.
 *
 * Single scale (infer_image, infer_images_batched).  The image is H x W, D = max(H, W); it was zero-padded at the bottom and right
 * to D x D and resized to S x S, so q is [S/4, S/4].  The plane is
 *     P = resize(q[:, :, None], (D, D), cubic=True)[:H, :W, 0]
 * with resize the dsize form of mpn_resize, scale (S/4) / D on both axes; only the H x W corner of the D x D grid is computed.
 *
 * Multi-scale + flip (infer_image_multiscale and its fused forms): _get_outputs applied to channel 18.  Per scale: q[:hp/4, :wp/4],
 * x4 up-sampling with the cubic mpn_resize (scale 0.25 exactly), crop to the unpadded (h, w), cubic mpn_resize to (H, W) in the
 * dsize form, times float32(1 / n), added into a float64 accumulator.  The pass over the mirrored image is accumulated separately
 * and read back at column W - 1 - x; a mask has no left/right twin, so no channel is permuted.
 *     P = float32((a_o + a_f) / 2)
 *
 * Mask.  M = 255 where P > thr, else 0, uint8.  The comparison is strict; a NaN gives 0.
 *
 * Score.  A byte is ON when it is non-zero.  Per image three int64 counts: inter, pred, gt; union = pred + gt - inter.  The summary is
 * formed on the host in float64 from the exact integers (evaluate/seg_eval.py: summarize_counts):
 *     iou = sum(inter) / sum(union);   mean_iou = mean of inter / union over the images with union > 0 (the others: n_empty);
 *     precision = sum(inter) / sum(pred);   recall = sum(inter) / sum(gt);   pixel_acc = sum(N - union + inter) / sum(N), N = H * W.
 *
 * The image table of mpn_segm_rasterize owns the MPN_SEGI_ prefix; the view table of mpn_seg_masks is MPN_SEGV_.
 * -------------------------------------------------------------------------------------------*/

/* mpn_seg_masks: mask (and optionally plane) of every image of a single-scale batch in one launch.
 * src: float32; the [Hs][Ws] map of image b is element (y, x) at src[SRC_OFF + y*sY + x*sX]; src_floats: floats readable from src.
 * imgs: int64 [n_img][MPN_SEGV_COLS] (device): float offset of the image's map in src; D, H, W; byte offset and row pitch of its
 *   H x W uint8 mask in `out`; float offset of its dense [H][W] plane in `planes` (ignored when planes is null).
 * out: uint8, out_bytes long.  planes: float32, plane_floats long, or null with plane_floats 0.
 * Grid: 64-column tiles up to max_w, 16-row tiles up to max_h, images.  A lane produces four consecutive pixels of a row and stores
 * their mask bytes as one word where the plane start and the pitch are multiples of 4 and the four lie inside the row, byte by byte
 * otherwise.  Every byte of every H x W plane is written, nothing between planes.  A row whose map leaves src, whose mask leaves
 * out, whose plane leaves planes, with D < max(H, W), H > max_h or W > max_w is skipped, never dereferenced.
 * MPN_E_BADARG before any HIP call: null or misaligned pointer, non-positive size or stride, n_img outside 1..65535, max_w / max_h
 * outside 1..65536, out_bytes / src_floats / plane_floats outside 1..2^40 (plane_floats != 0 without planes), src_floats too small for
 * one [Hs][Ws] map, or two of src, out, planes overlapping.  Nothing is allocated or synchronised. */
#define MPN_SEGV_SRC_OFF 0
#define MPN_SEGV_D 1
#define MPN_SEGV_H 2
#define MPN_SEGV_W 3
#define MPN_SEGV_OUT_OFF 4
#define MPN_SEGV_OUT_PITCH 5
#define MPN_SEGV_PLANE_OFF 6
#define MPN_SEGV_COLS 7
int mpn_seg_masks(const float* src, int64_t sY, int64_t sX, int Hs, int Ws, int64_t src_floats, const int64_t* imgs, int n_img,
                  int max_w, int max_h, float thr, uint8_t* out, int64_t out_bytes, float* planes, int64_t plane_floats,
                  void* stream);

/* mpn_tta_merge_mask: the multi-scale + flip merge of channel 18 in one launch.  scales: the HOST table of mpn_tta_merge with seg
 * pair maps: element (y, x, ch) at u[y*pitch + x*2 + ch], ch 0 from the pass over the original image, ch 1 from the pass over the
 * mirrored one, pitch >= 2 * rw, 1..8 scales.  With R and r as for mpn_tta_merge:
 *   a_o = sum over the table, in order, of (double)(R(U_s, y, x, 0) * r);   a_f = ... of (double)(R(U_s, y, W - 1 - x, 1) * r)
 *   P[y][x] = (float)((a_o + a_f) / 2);   M[y][x] = P[y][x] > thr ? 255 : 0
 * plane: dense float32 [H][W] or null; mask: uint8, row pitch mask_pitch >= W, or null; not both null.  No accumulator plane in
 * memory.  MPN_E_BADARG before any HIP call for a null table, both outputs null, n_scales outside 1..8, H or W outside 1..65536, a
 * pitch below 2 * rw, mask_pitch < W, or plane and mask overlapping. */
int mpn_tta_merge_mask(const MpnTtaScale* scales, int n_scales, int H, int W, float thr, float* plane, uint8_t* mask,
                       int64_t mask_pitch, void* stream);

/* mpn_mask_iou: counts[b] = (inter, pred, gt) of image b: the bytes that are non-zero in both planes, in the prediction, in the
 * ground truth.  imgs: int64 [n_img][MPN_MIOU_COLS] (device): H, W, then byte offset and row pitch of the plane in pred and in gt.
 * counts: int64 [n_img][3]; the call zeroes it on the stream and writes every element.  Lanes read 16 bytes where both plane starts
 * and pitches are multiples of 16, 8 where of 8, single bytes otherwise and in a row's tail.  Integer sums in registers, the wave,
 * LDS, then one integer atomic add per workgroup (32 rows of an image) and counter: the counts are identical on every run.
 * A row whose plane leaves its buffer or with H > max_h is skipped (its counts stay 0), never dereferenced.
 * MPN_E_BADARG before any HIP call: null or misaligned pointer, n_img outside 1..65535, max_h outside 1..65536, pred_bytes / gt_bytes
 * outside 1..2^40, counts overlapping pred or gt.  Nothing is allocated or synchronised. */
#define MPN_MIOU_H 0
#define MPN_MIOU_W 1
#define MPN_MIOU_PRED_OFF 2
#define MPN_MIOU_PRED_PITCH 3
#define MPN_MIOU_GT_OFF 4
#define MPN_MIOU_GT_PITCH 5
#define MPN_MIOU_COLS 6
int mpn_mask_iou(const uint8_t* pred, int64_t pred_bytes, const uint8_t* gt, int64_t gt_bytes, const int64_t* imgs, int n_img,
                 int max_h, int64_t* counts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pose-residual-network person assignment, device half (evaluate/tester.py:333-513; crop/gaussian helpers
 * datasets/coco_data/prn_gaussian.py:2,134-158).
 * mpn_prn_build_maps: for nboxes boxes (x, y, w, h doubles; box_img[b] = image of box b) and the heat-map peaks of their
 * images (peaks [n][2] doubles grouped by image then joint type; joint_off [nimg][18] offsets) builds
 *   occ    [nboxes][17][H][W] int32 : 1 + id of the peak assigned to the cell (id = position among its image's peaks), 0 = empty,
 *            with the reference's inside test, float64 cell arithmetic, one-branch clamp chain and overwrite order
 *            (tester.py:363-392); *err is set to 1 where the reference would raise IndexError;
 *   prn_in [nboxes][H][W][17] float32: the one-hot planes blurred by skimage.filters.gaussian (sigma 1, 'nearest', 9 taps;
 *            weights9 = the normalised kernel as scipy computes it), in scipy.ndimage.correlate1d's summation order.
 * mpn_prn_scores: score[b][t][y][x] (where occ > 0) = sum of the N x N window of prn_out[b][:, :, t] around (y, x), clipped
 * as prn_gaussian.crop does, in np.sum's own float32 order (pairwise over the row-major flattened window: exact ties between
 * candidates exist and the reference resolves them by sort order; tester.py:418-419); N odd, <= 15; argmax[b][t] = first row-major maximum of
 * the plane (tester.py:480).  H*W <= 4096.
 * Preconditions the entry points do not check: mpn_prn_build_maps refuses H*W > 4096 (MPN_E_UNSUPPORTED, nothing launched), but
 * mpn_prn_scores and mpn_prn_scores_compact do not look at H*W themselves — the caller keeps occ / prn_out / score at the size it
 * passes; and argmax[b][t] is defined only for a plane that holds a finite value or +inf: for a plane of nothing but -inf and NaN
 * no element compares greater than the initial -inf and the value written is not an index of the plane.
 * -------------------------------------------------------------------------------------------*/
int mpn_prn_build_maps(const double* peaks, const int32_t* joint_off, const double* boxes, const int32_t* box_img, int nboxes,
                       int H, int W, double in_thres, const double* weights9, int32_t* occ, float* prn_in, int32_t* err,
                       void* stream);
int mpn_prn_scores(const float* prn_out, const int32_t* occ, int nboxes, int H, int W, int N, float* score, int32_t* argmax,
                   void* stream);
/* mpn_prn_scores with a compact result (the full score / occupancy planes are 274 KB per box): per (box, joint type) the occupied
 * cells in row-major order — np.argwhere's order at tester.py:415 — as cand_id (peak id = occ - 1) and cand_score (window sum),
 * at most `cap` per plane (cand_n holds the true count; *overflow is set when one exceeds cap), plus the per-plane arg-max. */
int mpn_prn_scores_compact(const float* prn_out, const int32_t* occ, int nboxes, int H, int W, int N, int cap,
                           int32_t* cand_n, int32_t* cand_id, float* cand_score, int32_t* argmax, int32_t* overflow, void* stream);
/* HOST function (no device work, host pointers): the greedy (boxes x peaks) matching of tester.py:432-485 for a whole batch on the
 * compact candidate lists.  box_start [nimg+1]: the boxes of image i are box_start[i] .. box_start[i+1]; boxes (x, y, w, h);
 * joint_off / peaks as for mpn_prn_build_maps; out_kp [nb][17][3] (x, y, score) must be zero-filled.  Where the result would depend
 * on numpy's ordering of EQUAL positive scores, tie_flags[image*17 + type] is set and that pair is left to the caller. */
int mpn_prn_match_host(int nimg, const int32_t* box_start, const double* boxes, const int32_t* joint_off, const double* peaks,
                       const int32_t* cand_n, const int32_t* cand_id, const float* cand_score, int cap, const int32_t* argmax,
                       int H, int W, double* out_kp, uint8_t* tie_flags);

/* ---------------------------------------------------------------------------------------------
 * COCO keypoint AP / AR on the device (evaluate/tester.py:179-186: COCOeval(coco, res, 'keypoints') evaluate + accumulate; the
 * published algorithm restated, pycocotools is not linked).  All arithmetic float64.  Every pointer is a device pointer except
 * img_tab_host; doubles 8-byte aligned.  The caller builds the constant tables with numpy and passes them in: var [17] =
 * (2 sigma)^2, area_rng [n_area][2] (inclusive bounds), iou_thrs [n_thr], rec_thrs [n_rec].
 *
 * Images are described by img_tab [n_img + 1][4] int64, row i = (first detection, first ground truth, first kept detection,
 * first OKS element) of image i in ascending image-id order, row n_img = the totals (D, G, K, size of oks).  img_tab_host is the
 * same table in host memory: it is validated before any HIP call (row 0 zero, rows ascending, kept = min(detections, max_dets),
 * OKS block = kept x ground truths) and must equal the device copy the kernels read.
 *   det_kp [D][17][3] (x, y, anything), det_score [D] (finite): an image's detections in input order;
 *   gt_kp [G][17][3] (x, y, visibility), gt_area [G], gt_bbox [G][4] (x, y, w, h), gt_flags [G]: bit 0 = ignored (iscrowd or
 *   num_keypoints == 0), bit 1 = iscrowd.
 * mpn_oks_matrix (one launch, one workgroup per image): per image the stable descending-score order (ties: lower input index
 *   first) truncated to max_dets -> kept_src [K] (index into the D detections), kept_score [K], kept_area [K] = (max x - min x) *
 *   (max y - min y) over the detection's own 17 joints; oks [kept x G block per image, row-major, at the table's offsets] =
 *   mean over the joints with visibility > 0 of exp(-(dx^2 + dy^2) / var / (area + 2^-52) / 2), or, for a ground truth without a
 *   visible joint, over all 17 with dx, dy the distances to its box doubled about its centre.
 * mpn_oks_match (one launch, one wave per image x area range x threshold): COCOeval.evaluateImg.  gt_ig [n_area][G] = ignored or
 *   area outside [lo, hi]; det_match [n_area][n_thr][K] = matched ground truth (index into G) or -1; det_ig [n_area][n_thr][K] =
 *   the matched ground truth's ignore flag, or for an unmatched detection "own area outside [lo, hi]"; gt_match
 *   [n_area][n_thr][G] = the last kept detection (index into K) matched to the ground truth, or -1.
 * mpn_oks_accumulate (two launches): COCOeval.accumulate.  order [K] = kept detections in the stable descending-score order over
 *   all images (a rank sort: K^2 compares, no scratch); precision [n_thr][n_rec][n_area] and recall [n_thr][n_area], -1 where an
 *   area range has no non-ignored ground truth.  workspace: mpn_oks_eval_workspace_bytes(K, n_area, n_thr) bytes, contents need no
 *   initialisation.
 * MPN_E_BADARG before any HIP call: null pointer, n_img <= 0, max_dets outside 1..128, n_area outside 1..8, n_thr outside 1..64,
 * n_rec outside 1..4096, negative totals, a misaligned double array, a table that fails the checks above.
 * -------------------------------------------------------------------------------------------*/
int64_t mpn_oks_eval_workspace_bytes(int64_t n_kept, int n_area, int n_thr);
int mpn_oks_matrix(const double* det_kp, const double* det_score, const double* gt_kp, const double* gt_area,
                   const double* gt_bbox, const int64_t* img_tab_host, const int64_t* img_tab, int n_img, int max_dets,
                   const double* var, int32_t* kept_src, double* kept_score, double* kept_area, double* oks, void* stream);
int mpn_oks_match(const double* oks, const double* kept_area, const double* gt_area, const int32_t* gt_flags,
                  const int64_t* img_tab_host, const int64_t* img_tab, int n_img, int max_dets, const double* area_rng,
                  int n_area, const double* iou_thrs, int n_thr, int32_t* det_match, int32_t* det_ig, int32_t* gt_ig,
                  int32_t* gt_match, void* stream);
int mpn_oks_accumulate(const double* kept_score, const int32_t* det_match, const int32_t* det_ig, const int32_t* gt_ig,
                       int64_t n_kept, int64_t n_gt, int n_area, int n_thr, const double* rec_thrs, int n_rec,
                       int32_t* order, double* precision, double* recall, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * COCO box AP / AR on the device (COCOeval(coco, res, 'bbox') evaluate + accumulate: pycocotools cocoeval.py computeIoU /
 * evaluateImg / accumulate and maskApi.c:bbIou, the published algorithm restated, pycocotools is not linked; the reference scores
 * its detection subnet by validation loss only, evaluate/tester.py:515-543).  All arithmetic float64 and only + - * / min max, so
 * every result equals a numpy restatement bit for bit.  Every pointer is a device pointer except tab_host, cat_tab_host and
 * max_dets_host; doubles and int64 tables 8-byte aligned.
 *
 * A row is one (category, image) pair that has at least one detection or ground truth; rows are ordered category-major, then by
 * ascending image id.  tab [n_row + 1][4] int64, row i = (first detection, first ground truth, first kept detection, first IoU
 * element), row n_row = the totals (D, G, K, size of iou): the convention of img_tab above, validated on the host the same way.
 * cat_tab [n_cat + 1][2] int64 = (first kept detection, first ground truth) of every category, last row (K, G).
 *   det_box [D][4], gt_box [G][4]: (x, y, w, h); det_score [D] (finite); gt_flags [G]: bit 0 = ignored, bit 1 = iscrowd.
 * mpn_box_iou_matrix (one launch, one workgroup per row): the row's stable descending-score order (ties: lower input index
 *   first) truncated to max_dets -> kept_src [K] (index into the D detections), kept_score [K], kept_area [K] = w * h of the
 *   detection's own box, kept_rank [K] = position inside the row; iou [kept x G block per row, row-major, at the table's offsets]
 *   as maskApi.c:bbIou: w = min(D.x + D.w, G.x + G.w) - max(D.x, G.x), 0 when w <= 0, h likewise, i = w * h,
 *   u = crowd ? D.w * D.h : D.w * D.h + G.w * G.h - i, iou = i / u.
 * The matching is mpn_oks_match on (iou, kept_area, the annotations' area fields, gt_flags, tab).
 * mpn_box_accumulate (two launches): COCOeval.accumulate.  order [K] = every category's kept detections in the stable
 *   descending-score order over its rows (a segmented rank sort, no scratch); precision [n_thr][n_rec][n_cat][n_area][n_max] and
 *   recall [n_thr][n_cat][n_area][n_max] over the detections with kept_rank < max_dets_host[m], -1 where the category has no
 *   non-ignored ground truth in the area range.  det_match / det_ig / gt_ig as mpn_oks_match wrote them.  workspace:
 *   mpn_box_eval_workspace_bytes(K, n_area, n_max, n_thr) bytes, contents need no initialisation.
 * MPN_E_BADARG before any HIP call: null pointer, n_row <= 0, max_dets (and every max_dets_host entry) outside 1..128, n_cat
 * outside 1..65535, n_area outside 1..8, n_max outside 1..4, n_thr outside 1..64, n_rec outside 1..4096, negative totals, a
 * misaligned double array, a table that fails the checks above.
 * -------------------------------------------------------------------------------------------*/
int64_t mpn_box_eval_workspace_bytes(int64_t n_kept, int n_area, int n_max, int n_thr);
int mpn_box_iou_matrix(const double* det_box, const double* det_score, const double* gt_box, const int32_t* gt_flags,
                       const int64_t* tab_host, const int64_t* tab, int n_row, int max_dets, int32_t* kept_src,
                       double* kept_score, double* kept_area, int32_t* kept_rank, double* iou, void* stream);
int mpn_box_accumulate(const double* kept_score, const int32_t* kept_rank, const int32_t* det_match, const int32_t* det_ig,
                       const int32_t* gt_ig, const int64_t* cat_tab_host, const int64_t* cat_tab, int n_cat, int64_t n_kept,
                       int64_t n_gt, int n_area, int n_thr, const int32_t* max_dets_host, int n_max, const double* rec_thrs,
                       int n_rec, int32_t* order, double* precision, double* recall, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPN_H_ */
