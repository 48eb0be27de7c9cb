/*
 * texpose_amd.h -- C ABI of the MI355X (gfx950) ray-marching library.
 *
 * Drop-in boundary: the reference has no FFI; its boundary is the Python
 * class protocol  Graph.render / NeRF.composite / RaySampler.get_rays ...  selected by module
 * name (reference train.py:18-19, model/base.py:42-44).  texpose_amd/ mirrors that protocol in
 * Python and reaches the GPU only through the entry points below (ctypes, see
 * texpose_amd/_lib.py and INTEGRATION.md).  Every pointer is a DEVICE pointer unless noted,
 * every tensor is dense row-major fp32, indices are int64, `stream` is a hipStream_t.
 * Launchers only enqueue work on `stream`: no allocation, no synchronisation, graph-capturable.
 *
 * Return value: 0 on success, a hipError_t (>0) when the launch failed, <0 for invalid
 * arguments.  tp_last_error() returns a static, thread-local description.
 *
 * "ref:" comments cite the reference file:line each entry point replaces.
 */
#ifndef TEXPOSE_AMD_H
#define TEXPOSE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* tp_stream_t; /* hipStream_t */

#define TP_ABI_VERSION 16

int tp_abi_version(void);
const char* tp_last_error(void);

/* ------------------------------------------------------------------------------------------
 * K1  fused ray generation + depth bounds + stratified samples
 * ref: tools/ray_sampler.py:24-69 (train rays/bounds), camera.py:292-314 +
 *      model/nerf_adapt_st_gan.py:573-579,702-710 (eval rays + row gather),
 *      camera.py:415-433 / compute_box.py:69-87,270-272 + data/lm.py:349-350 (AABB bounds),
 *      model/nerf_adapt_st_gan.py:683-700 (sample_depth).
 * ------------------------------------------------------------------------------------------ */
enum tp_pixel_mode {
  TP_PIX_COORDS = 0, /* train: coords [B,R,2] in [-1,1] (x,y); u,v = bilinear index-grid lookup */
  TP_PIX_INDEX = 1   /* eval : ray_idx [B,R] int64 row-major pixel index; u,v = col+.5,row+.5 */
};
enum tp_bounds_mode {
  TP_BOUNDS_MAP = 0,  /* z_near/z_far [B,H*W] maps: bilinear (coords) or gathered (index) */
  TP_BOUNDS_AABB = 1, /* in-kernel slab test against aabb_min/aabb_max, misses -> bg range */
  TP_BOUNDS_NONE = 2  /* rays only: near/far/depth outputs untouched */
};
enum tp_jitter_mode {
  TP_JITTER_MID = 0,    /* sample_stratified=false: 0.5 */
  TP_JITTER_GIVEN = 1,  /* rand [B,R,N] supplied by the caller (parity runs) */
  TP_JITTER_PHILOX = 2  /* in-kernel Philox4x32-10 keyed by (seed, offset) */
};
enum tp_depth_param {   /* options nerf.depth.param (model/nerf_adapt_st_gan.py:699) */
  TP_DEPTH_METRIC = 0,
  TP_DEPTH_INVERSE = 1  /* 1 / (sample + 1e-8) */
};

typedef struct tp_raygen_args {
  const float* intr;      /* [B,3,3] */
  const float* pose;      /* [B,3,4] object->camera [R|t] */
  const float* coords;    /* [B,R,2] (TP_PIX_COORDS) or NULL */
  const int64_t* ray_idx; /* [B,R]   (TP_PIX_INDEX)  or NULL */
  const float* z_near;    /* [B,H*W] (TP_BOUNDS_MAP) or NULL */
  const float* z_far;     /* [B,H*W] */
  const float* rand;      /* [B,R,N] (TP_JITTER_GIVEN) or NULL */
  float aabb_min[3];      /* TP_BOUNDS_AABB (host values) */
  float aabb_max[3];
  float bg_near, bg_far;  /* TP_BOUNDS_AABB fallback range */
  const float* valid_rect; /* TP_BOUNDS_AABB, optional: [B,4] device (x0,y0,x1,y1) in pixel coordinates of the H x W image;
                            * pixels whose centre (col+0.5,row+0.5 / bilinear coordinate) lies outside get the fallback
                            * range.  Reproduces the zero padding of the stored bound maps when a detection crop leaves
                            * the camera frame (data/lm.py:455-495 Crop_by_Pad, :349-350).  NULL = no rectangle. */
  uint64_t seed, offset;  /* TP_JITTER_PHILOX */
  const uint64_t* offset_dev; /* TP_JITTER_PHILOX, optional: a device word ADDED to offset (the step counter of a captured training
                               * step: the same launch draws different numbers at every replay) */
  int B, R, H, W, N;      /* N = samples per ray (0: no depth output) */
  int pixel_mode, bounds_mode, jitter_mode;
  int ndc;                /* non-zero: centre / ray re-expressed in normalised device coordinates, near plane z = 1 (camera.py:325-342
                           * convert_NDC; model/nerf_adapt_st_gan.py:581-583 `camera.ndc`).  Applied AFTER the bounds, which the reference
                           * takes from the metric rays. */
  int depth_param;        /* TP_DEPTH_METRIC, or TP_DEPTH_INVERSE: depth = 1 / (sample + 1e-8) (model/nerf_adapt_st_gan.py:699) */
  float* center;          /* [B,R,3] out */
  float* ray;             /* [B,R,3] out (camera-z component == 1 unless ndc) */
  float* near;            /* [B,R] out, may be NULL */
  float* far;             /* [B,R] out, may be NULL */
  float* depth;           /* [B,R,N] out, may be NULL */
} tp_raygen_args;

int tp_raygen(const tp_raygen_args* args /* host struct */, tp_stream_t stream);

/* The ray generation of a TRAINING step with the two small launches in front of it folded in (a captured iteration is a chain of
 * dependent launches: each one fewer is ~5 us of it).  `sampler` (or NULL): the launch draws the patch coordinates itself -- the
 * arguments of tp_patch_coords (K13; tools/patch_sampler.py:64-114), ray q = element q of the B x p x p grid, R == p * p,
 * args->pixel_mode TP_PIX_COORDS, args->coords ignored -- and writes them to sampler->coords / ->scales for the later consumers.
 * `rows` (or NULL): extra workgroups gather the per-image latent rows (the arguments of tp_latent_rows_fwd).  Same values as the
 * separate launches, bit for bit. */
typedef struct tp_patch_sampler_job {
  const float* u;          /* [3,B] uniforms, or NULL: drawn in the kernel from (seed, *counter) */
  int p;
  const float* lattice;    /* [p] linspace(-1, 1, p) */
  const float* lo_dev;     /* device word, or NULL: lo_host */
  float lo_host, span_host, hi;
  int random_scale, random_shift;
  uint64_t seed;
  const uint64_t* counter;
  float* coords;           /* [B,p,p,2] out */
  float* scales;           /* [B] out */
} tp_patch_sampler_job;
typedef struct tp_latent_rows_job {
  const float* w_trans; const float* w_light; const int64_t* idx;
  int B, C_trans, C_light;
  float* out_trans; float* out_light; int64_t* idx_copy /* or NULL */;
} tp_latent_rows_job;
int tp_raygen_train(const tp_raygen_args* args, const tp_patch_sampler_job* sampler, const tp_latent_rows_job* rows, tp_stream_t stream);

/* Standalone slab test (camera.py:415-433): o,d [n,3] -> t_near,t_far [n], valid [n] (uint8). */
int tp_aabb(const float* aabb_min3 /*host*/, const float* aabb_max3 /*host*/, const float* o, const float* d,
            int64_t n, float* t_near, float* t_far, uint8_t* valid, tp_stream_t stream);

/* Standalone Graph.sample_depth (model/nerf_adapt_st_gan.py:683-700): near,far [n] -> depth [n,N]. */
int tp_sample_depth(const float* near, const float* far, const float* rand /*[n,N] or NULL*/, int jitter_mode,
                    uint64_t seed, uint64_t offset, int64_t n, int N, int depth_param /* TP_DEPTH_* */, float* depth, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K2/K3  positional encoding + static/transient/light MLP
 * ref: layers/nerf_static_transient_light.py:76-145 (forward), :147-166 (forward_samples),
 *      :217-234 (positional_encoding), camera.py:317-322 (points from depth).
 * Architecture is the reference default (options/nerf_lm_adapt_gan.yaml:9-17,37-40): width 256,
 * 8 trunk layers with skip at 4, L_3D=10, L_view=4, 16 transient + 48 light latents.
 * ------------------------------------------------------------------------------------------ */

/* Pointers to the reference state-dict tensors, device memory, W [out,in]. */
typedef struct tp_mlp_weights {
  const float* feat_w[8];  const float* feat_b[8];   /* mlp_feat.{0..7}   */
  const float* rgb_w[4];   const float* rgb_b[4];    /* mlp_rgb.{0..3}    */
  const float* trans_w[4]; const float* trans_b[4];  /* mlp_trans.{0..3}  */
} tp_mlp_weights;

/* Size in bytes of the packed (MFMA-fragment-ordered, streaming-ordered) weight image. */
size_t tp_mlp_packed_bytes(void);
/* Which parts to (re)pack: the trunk is frozen, the heads change every optimiser step. */
enum { TP_PACK_TRUNK = 1, TP_PACK_HEADS = 2, TP_PACK_ALL = 3,
       TP_PACK_F16X3 = 4 /* OR-ed in: build the split-fp16 (hi+lo) stream of the TP_MLP_F16X3 forward; same size */,
       TP_PACK_RAYBIAS = 8 /* OR-ed in with TP_PACK_F16X3 or TP_PACK_F16: the stream variant of tp_mlp_fwd_args.ray_bias (same buffer size) */,
       TP_PACK_F16 = 16 /* OR-ed in: build the single-fp16 stream of the TP_MLP_F16 forward (inference only); same buffer size */ };
int tp_mlp_pack(const tp_mlp_weights* w /*host struct of device ptrs*/, int parts, void* packed, tp_stream_t stream);
/* Training (TP_MLP_F16X3): everything that is rebuilt from the HEAD weights after an optimiser step, in one launch: the head chunks
 * and head biases of the f16x3 forward stream `packed` (what tp_mlp_pack(TP_PACK_HEADS | TP_PACK_F16X3) writes) and, when packed_t is
 * not NULL, the transposed f16x3 image tp_mlp_bwd streams (what it builds itself when called with repack != 0). */
int tp_mlp_pack_heads_f16x3(const tp_mlp_weights* w, void* packed, void* packed_t, tp_stream_t stream);
/* Same image built on the host from HOST weight pointers (no GPU needed; used by the CPU tests). */
int tp_mlp_pack_host(const tp_mlp_weights* w_host, float* packed_host);

/* Bytes of scratch the forward needs for a given launch (per-workgroup spill of the trunk feature). */
size_t tp_mlp_workspace_bytes(int64_t n_samples);
/* Bytes of the optional activation record kept for the backward pass (7 x 256 floats / sample,
 * rounded up to whole 128-sample tiles). */
size_t tp_mlp_saved_bytes(int64_t n_samples);

typedef struct tp_mlp_fwd_args {
  const void* packed;      /* tp_mlp_pack output */
  /* input form A (forward_samples): center,ray [B,R,3], depth [B,R,N] */
  const float* center; const float* ray; const float* depth;
  /* input form B (NeRF.forward): points, ray_unit [B,R,N,3]; used when center == NULL */
  const float* points; const float* ray_unit;
  const float* lat_trans;  /* [B,16] */
  const float* lat_light;  /* [B,48] */
  int B, R, N;
  float* rgb;              /* [B,R,N,3,2] out (last dim: static, transient) */
  float* density;          /* [B,R,N,2]   out */
  float* uncert;           /* [B,R,N,1]   out */
  float* saved;            /* optional activations for tp_mlp_bwd (tp_mlp_saved_bytes) or NULL */
  void* workspace;         /* tp_mlp_workspace_bytes */
  int precision;           /* TP_MLP_FP32 (exact fp32 MFMA), TP_MLP_F16X3 (packed with TP_PACK_F16X3) or TP_MLP_F16 (packed with
                              TP_PACK_F16; no `saved`, no `density_noise`: inference only) */
  int* status;             /* TP_MLP_F16X3 / TP_MLP_F16: device word, bit 0 is set if an activation left the fp16 range */
  unsigned int* act_max;   /* TP_MLP_F16X3 / TP_MLP_F16, optional (may be NULL): device word that receives, by atomic max, the fp32 bit
                              pattern of the largest hidden activation handed to the matrix cores in this call (post-ReLU,
                              its fp16 hi part: 11 significant bits).  The range guard fires at 6e4; this word says how far
                              below it a network runs.  Zero it before the calls to be covered. */
  float* ray_bias;         /* optional (NULL = off).  TP_MLP_F16X3 or TP_MLP_F16 without `saved`, input form A, N % 128 == 0 (every
                              128-sample tile lies inside one ray), `packed` built with TP_PACK_F16X3 (TP_PACK_F16) | TP_PACK_RAYBIAS: device scratch of
                              tp_mlp_ray_bias_bytes(B, R).  The inputs of mlp_rgb.0 that are constant along a ray (view encoding 27,
                              light code 48 of its 334 columns; reference layers/nerf_static_transient_light.py:104-118) and the
                              transient code of mlp_trans.0 (:127-129) are then contracted once per ray / image in fp32 by a
                              pre-kernel and enter the layer as a per-ray bias instead of 96 input columns of every sample. */
  const float* density_noise; /* optional (NULL = off), [B*R*N]: added to the STATIC density's pre-activation before its softplus
                              (reference nerf.density_noise_reg, layers/nerf_static_transient_light.py:96-97, train mode: the caller
                              passes randn * density_noise_reg).  Not with `ray_bias`. */
} tp_mlp_fwd_args;
size_t tp_mlp_ray_bias_bytes(int B, int R);
/* TP_MLP_F16X3: every fp32 operand is split into hi + lo fp16 (22-bit significand) and hi*hi + hi*lo + lo*hi is
 * accumulated in fp32 on the f16 matrix cores (16x the fp32-MFMA rate / 3).  Measured error vs an fp64 oracle is
 * within 1.3x of plain fp32.  Requires |activation| < 6e4 (see `status`) and |weight| < 2^8 (the stream
 * holds W * 2^8 in fp16; a larger weight overflows, unflagged).  The 1.3x holds while the lo halves are normal fp16 numbers: where a
 * layer's weights all lie below ~2^-11 or its activations all below 2^-3, the contract is rtol 1e-4 / atol 1e-6 of fp32 and 32x
 * fp32's error (measured up to 18x).  With `saved` it writes
 * the same fp32 activation record as TP_MLP_FP32 (the backward kernels do not depend on how the forward was computed). */
/* TP_MLP_F16 (inference only, not fp32-grade): ONE fp16 product per multiply-add with fp32 accumulation on the f16 matrix cores,
 * 3x fewer MFMAs than TP_MLP_F16X3 and half the weight stream.  The 256-wide layers (trunk, hidden layers of both heads, and the
 * encoding / latent inputs that feed them) use weights rounded to fp16 (nearest even) once at pack time and activations rounded
 * to fp16 (nearest even) as they are consumed -- about 2^-11 relative per operand.  The narrow output layers (density, transient,
 * rgb) and the per-ray bias pre-kernels keep the TP_MLP_F16X3 arithmetic.  Range guard as TP_MLP_F16X3 (`status`, `act_max`). */
enum { TP_MLP_FP32 = 0, TP_MLP_F16X3 = 1, TP_MLP_F16 = 2 };

int tp_mlp_fwd(const tp_mlp_fwd_args* args, tp_stream_t stream);

/* Backward of the two trainable heads (autograd of layers/...light.py:102-137; the trunk is frozen,
 * :34,87-100).  Consumes the activation record of a forward run with `saved` != NULL on the same
 * (B,R,N).  When B*R*N is not a multiple of 128 the caller must zero the last tile's part of `saved`
 * BEFORE the forward (the weight-gradient GEMM contracts whole 32-sample groups).  At most 32 images
 * per call.  All gradient outputs are overwritten (not accumulated); results are deterministic
 * (fixed-order split-K reduction, no float atomics). */
size_t tp_mlp_packed_t_bytes(void);                 /* scratch for the transposed head-weight stream */
size_t tp_mlp_bwd_workspace_bytes(int64_t n_samples);
typedef struct tp_mlp_bwd_args {
  tp_mlp_weights weights;  /* rgb_w[0..3], trans_w[0..3] are read (device pointers) */
  void* packed_t;          /* tp_mlp_packed_t_bytes; rebuilt from `weights` when repack != 0 */
  int repack;
  const float* saved;      /* record written by tp_mlp_fwd */
  const float* rgb; const float* density; const float* uncert;        /* forward outputs */
  const float* g_rgb; const float* g_density; const float* g_uncert;  /* their cotangents */
  const float* lat_trans;  /* [B,16] */
  const float* lat_light;  /* [B,48] */
  int B, R, N;
  float* g_rgb_w[4];   float* g_rgb_b[4];     /* out: same shapes as mlp_rgb.{i}.weight / bias   */
  float* g_trans_w[4]; float* g_trans_b[4];   /* out: same shapes as mlp_trans.{i}.weight / bias */
  float* g_lat_trans;  /* [B,16] out */
  float* g_lat_light;  /* [B,48] out */
  void* workspace;         /* tp_mlp_bwd_workspace_bytes */
  int wgrad_precision;     /* arithmetic of the backward GEMMs (dgrad and wgrad).  TP_MLP_FP32: exact fp32 MFMA;
                              TP_MLP_F16X3: split-fp16 products with power-of-two scaling of the gradients (fp32-grade;
                              requires |activation| < 6e4, i.e. a record written by a TP_MLP_F16X3 forward whose status
                              word stayed clear; `packed_t` is then built in the transposed f16x3 format) */
  int dz_max_is_clear;     /* TP_MLP_F16X3: the scale word inside `workspace` is known to be zero -- true after any completed call
                              with the same workspace and B*R*N (the call's last kernel clears it) -- so the call does not
                              memset it.  0 = clear it first (always safe). */
  int wgrad_cus;           /* TP_MLP_F16X3: compute units the weight-gradient launch fills (one workgroup each; its split-K slice
                              counts follow).  0 = all.  A caller that runs other streams beside this call (the captured GAN
                              iteration: the discriminator step) passes 7/8 of the device so that their launches are not starved
                              for the length of the weight gradient; values are identical for every choice up to the order of
                              the fixed-order split-K sums. */
} tp_mlp_bwd_args;
int tp_mlp_bwd(const tp_mlp_bwd_args* args, tp_stream_t stream);

/* Standalone positional encoding (layers/...light.py:217-234): x [n,C] -> [n, 2*C*L]. */
int tp_posenc(const float* x, int64_t n, int C, int L, float* out, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K4  per-ray alpha composite
 * ref: layers/nerf_static_transient_light.py:168-212
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_composite_args {
  const float* ray;      /* [n,3]     */
  const float* rgb;      /* [n,N,3,2] */
  const float* density;  /* [n,N,2]   */
  const float* depth;    /* [n,N]     */
  const float* uncert;   /* [n,N]     */
  int64_t n; int N; float min_uncert;
  float* out_ray;        /* [n,14]: rgb3 rgb_static3 rgb_transient3 depth opacity opacity_static opacity_transient uncert */
  float* alpha_static;   /* [n,N] or NULL */
  float* alpha_transient;/* [n,N] or NULL */
  float* prob;           /* [n,N] or NULL */
  float* rgb_ray;        /* [n,3] or NULL: compact copy of out_ray[:,0:3] (what the losses and the PatchGAN consume) */
  float* uncert_ray;     /* [n]   or NULL: compact copy of out_ray[:,13] */
} tp_composite_args;
int tp_composite_fwd(const tp_composite_args* args, tp_stream_t stream);

typedef struct tp_composite_bwd_args {
  tp_composite_args fwd;        /* same inputs as the forward (outputs ignored) */
  const float* g_out_ray;       /* [n,14] cotangent of out_ray, or NULL (zeros) when g_rgb_ray / g_uncert_ray carry it all */
  const float* g_alpha_static;  /* [n,N] or NULL */
  const float* g_alpha_transient;
  const float* g_prob;
  float* g_rgb;                 /* [n,N,3,2] out */
  float* g_density;             /* [n,N,2]   out */
  float* g_uncert;              /* [n,N]     out */
  const float* g_rgb_ray;       /* [n,3] or NULL: cotangent of rgb_ray, ADDED to g_out_ray[:,0:3] */
  const float* g_uncert_ray;    /* [n]   or NULL: cotangent of uncert_ray, ADDED to g_out_ray[:,13] */
  const float* g_rgb_ray2;      /* [n,3] or NULL: two more cotangents of rgb_ray (one per consumer of the colours), added likewise */
  const float* g_rgb_ray3;
  const float* g_density_add;   /* [n,N,2] or NULL: a second cotangent of the densities, ADDED to g_density */
} tp_composite_bwd_args;
int tp_composite_bwd(const tp_composite_bwd_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * One-call evaluation render: tp_raygen -> tp_mlp_fwd -> tp_composite_fwd on one stream
 * ref: Graph.render with mode != 'train', model/nerf_adapt_st_gan.py:547-631 (latent rows chosen by the caller, :589-605)
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_render_eval_args {
  tp_raygen_args raygen;   /* inputs, sizes and modes as for tp_raygen (N > 0); its output pointers are ignored */
  const void* packed;      /* tp_mlp_pack output for `precision` */
  const float* lat_trans;  /* [B,16] */
  const float* lat_light;  /* [B,48] */
  int precision;           /* TP_MLP_FP32, TP_MLP_F16X3 or TP_MLP_F16 */
  int* status;             /* as in tp_mlp_fwd_args (may be NULL) */
  float min_uncert;
  void* workspace;         /* tp_render_eval_workspace_bytes(B, R, N) */
  float* out_ray;          /* [B*R,14] out, layout of tp_composite_args.out_ray */
  float* alpha_static;     /* [B*R,N] out or NULL */
  float* alpha_transient;  /* [B*R,N] out or NULL */
  int packed_ray_bias;     /* non-zero: `packed` is the TP_PACK_F16X3 (TP_PACK_F16) | TP_PACK_RAYBIAS stream (precision TP_MLP_F16X3
                              or TP_MLP_F16, N % 128 == 0) and
                              the MLP runs in its ray-bias form (tp_mlp_fwd_args.ray_bias; the scratch is part of `workspace`) */
} tp_render_eval_args;
size_t tp_render_eval_workspace_bytes(int B, int R, int N);   /* (includes the ray-bias scratch) */
int tp_render_eval(const tp_render_eval_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K5  patch gather for the photometric / PatchGAN inputs
 * ref: model/nerf_adapt_st_gan.py:444-461,516-545,726-745 (8 grid_sample calls per step)
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_patch_gather_args {
  const float* coords;     /* [B,P,2] (x,y) in [-1,1], P = p*p */
  const float* image;      /* [B,3,H,W] */
  const float* image_syn;  /* [B,3,H,W] */
  const float* nocs;       /* [B,3,H,W] */
  const float* normal;     /* [B,3,H,W] */
  const float* obj_mask;   /* [B,H,W]   (binarised > 0 in-kernel) */
  const float* mask_syn;   /* [B,H,W]   */
  int B, P, H, W;
  float* out;              /* [B,14,P]: image3 image_syn3 nocs3*mask_syn normal3*mask_syn mask mask_syn */
  /* optional (disc_rgb != NULL): the PatchGAN's input stacks of the same pixels in the same launch, what tp_disc_inputs forms from
   * `out` and the rendered colours disc_rgb [B,P,3]: disc_real / disc_fake [B, disc_geo ? 9 : 3, P] (model/nerf_adapt_st_gan.py:478-497) */
  const float* disc_rgb; float* disc_real; float* disc_fake; int disc_geo; int pad_;
} tp_patch_gather_args;
int tp_patch_gather(const tp_patch_gather_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K6  evaluation metrics after the render: squared-error and SSIM sums (PSNR / SSIM of evaluate_full)
 * ref: model/nerf_adapt_st_gan.py:340-362, external/pohsun_ssim/pytorch_ssim/__init__.py:7-37
 *      (the optional 480x640 resize of :346-350 is fused: bilinear align_corners=False / nearest)
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_eval_metrics_args {
  const float* rgb_static; /* [B,h*w,3] the render (channels last, as Graph.render returns it) */
  const float* image;      /* [B,3,h,w] */
  const float* obj_mask;   /* [B,h,w]   multiplies the image (NOT binarised: the reference uses it as is) */
  int B, h, w;
  int out_h, out_w;        /* metric resolution; == (h, w) for no resize */
  void* workspace;         /* tp_eval_metrics_workspace_bytes(B, out_h, out_w) */
  double* out;             /* [B,2]: sum over 3*out_h*out_w of squared error, of the SSIM map */
} tp_eval_metrics_args;
int64_t tp_eval_metrics_workspace_bytes(int B, int out_h, int out_w);
int tp_eval_metrics(const tp_eval_metrics_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K7  spectral-norm weight normalisation for all convolutions of the PatchGAN at once
 * ref: torch.nn.utils.spectral_norm as applied in layers/discriminator.py:45-115 (one power iteration per forward in
 *      training mode: v <- normalize(W^T u), u <- normalize(W v), sigma = u.(W v), W_sn = W / sigma; u, v in place)
 * ------------------------------------------------------------------------------------------ */
#define TP_SN_MAX_WEIGHTS 8
#define TP_SN_MAX_SLABS 8        /* rows <= 512 */
#define TP_SN_MAX_SETS 3         /* power iterations tp_sn_fwd_sets runs in a row */
typedef struct tp_sn_weight {
  const float* weight;     /* [rows,cols] = weight_orig.view(out, -1); fwd only */
  float* u;                /* [rows]  updated in place when training */
  float* v;                /* [cols]  updated in place when training */
  float* weight_sn;        /* [rows,cols] fwd: out; bwd: in */
  float* sigma;            /* [1]     fwd: out; bwd: in */
  const float* grad_sn;    /* [rows,cols] bwd: gradient wrt weight_sn */
  float* grad;             /* [rows,cols] bwd: out, gradient wrt weight */
  float* work;             /* tp_sn_work_floats(rows, cols) floats of scratch */
  int rows, cols;
  float* u_out;            /* fwd, optional: copy of u [rows] as it stands AFTER this call's power iteration (the backward of
                              THIS forward needs it; later forwards of the iteration advance u / v in place) */
  float* v_out;            /* fwd, optional: copy of v [cols] likewise */
  int32_t accumulate;      /* bwd: grad += */
  /* bwd, optional: a SECOND normalised instance of the same weight in one optimiser step (the discriminator step's fake pass:
   * the power iteration advances between the passes) -- grad = f(grad_sn, weight_sn, u, v, sigma) + f(grad_sn2, ...) in the same
   * two launches; all five or none */
  const float* grad_sn2; const float* weight_sn2; const float* u2; const float* v2; const float* sigma2;
} tp_sn_weight;
int64_t tp_sn_work_floats(int rows, int cols);
/* three launches (two in eval mode): every workgroup of the consuming kernel normalises v / u for itself */
int tp_sn_fwd(const tp_sn_weight* weights, int n, int training, tp_stream_t stream);
/* n_sets training-mode forwards in a row (entry k * n + i = weight i of set k: own weight_sn / sigma / u_out / v_out; weight, u, v, work
 * shared): two launches per set and ONE normalisation launch for all sets; bit-identical to n_sets tp_sn_fwd calls. */
int tp_sn_fwd_sets(const tp_sn_weight* weights, int n, int n_sets, tp_stream_t stream);
int tp_sn_bwd(const tp_sn_weight* weights, int n, tp_stream_t stream);
/* tp_sn_bwd for a discriminator step that ENDS here (one rank, no gradient reduction behind it): the loss total + step gate ride in the
 * first launch (what tp_weighted_sum_flags does: total = sum_k terms[k][0] * weights[k] in ascending k, bad[word_finite] |= 1 if it is not
 * finite, snapshot[0..n_bad) = bad[...]), the RMSprop step of every weight (tp_rmsprop_step's arithmetic; withheld if a snapshot word is
 * set) in the second, on the gradient element the thread has just formed -- 2 launches instead of 4.  The gradients are still written.
 * ref: model/nerf_adapt_st_gan.py:129-171 (disc_trainstep: summarize_loss, backward, optim_disc.step()), model/base.py:145-157 */
typedef struct tp_sn_step_tail {
  const float* terms[4]; float weights[4]; int n_terms; int word_finite;
  float* total;                                  /* [1] */
  int32_t* bad; int32_t* snapshot; int n_bad; int pad_;
  float* param[TP_SN_MAX_WEIGHTS];               /* weight_orig of weight i (the tensor tp_sn_weight.grad belongs to) */
  float* square_avg[TP_SN_MAX_WEIGHTS];
  float* step[TP_SN_MAX_WEIGHTS];                /* optional 0-dim float32 counters, += 1 per applied step */
  const float* lr_dev; float lr_host, alpha, one_minus_alpha, eps;      /* (one_minus_alpha = (float)(1.0 - alpha) formed in double, like tp_rmsprop_step) */
} tp_sn_step_tail;
int tp_sn_bwd_step(const tp_sn_weight* weights, int n, const tp_sn_step_tail* tail, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K8  render-consuming loss terms of the generator step (render, uncert, trans_reg) and their gradients
 * ref: model/nerf_adapt_st_gan.py:712-776 (compute_loss, train_step == 'nerf', nerf.mask_obj)
 * ------------------------------------------------------------------------------------------ */
#define TP_NERF_LOSSES_MAX_BLOCKS 1024
typedef struct tp_nerf_losses_args {
  const float* rgb;        /* [B,P,3]   composite output */
  const float* uncert;     /* [B,P]     composite output (>= min_uncert) */
  const float* density;    /* [B,P,N,2] MLP output; [...,1] = sigma_transient */
  const float* gathered;   /* [B,14,P]  tp_patch_gather output: image = channels 0..2, object mask = channel 12 */
  int B, P, N;
  void* workspace;         /* 4 * TP_NERF_LOSSES_MAX_BLOCKS floats */
  double* sums;            /* [4]: sum m*se/u^2, sum m, sum log u^2, sum sigma_t  (fwd: out, bwd: in) */
  float* losses;           /* fwd, optional [3]: render = s0 / (s1 + 1e-5), uncert = 5 + s2 / (B P) / 2, trans_reg = s3 / (B P N)
                              in fp32 from the fp32-rounded sums, the reference's operation order */
  uint32_t* ticket;        /* fwd: ONE zero-filled device word owned by the calling stream (the arrival counter of the last-block
                              reduction; the launch leaves it zero).  Launches that may overlap -- different streams of one device --
                              need different words; launches on one stream may share one.  Unused by the backward. */
} tp_nerf_losses_args;
int tp_nerf_losses_fwd(const tp_nerf_losses_args* args, tp_stream_t stream);
/* g_render / g_unc / g_trans: the upstream gradients of the three terms, one device scalar each (NULL = 0) */
int tp_nerf_losses_bwd(const tp_nerf_losses_args* args, const float* g_render, const float* g_unc, const float* g_trans,
                       float* g_rgb, float* g_uncert, float* g_density, tp_stream_t stream);
/* the same launch + the generator step's loss total and step gate (tp_weighted_sum_flags' arguments and arithmetic) as a side job of its
 * first thread: one launch less on the render's backward chain (model/base.py:145-157 summarize_loss) */
int tp_nerf_losses_bwd_total(const tp_nerf_losses_args* args, const float* g_render, const float* g_unc, const float* g_trans,
                             float* g_rgb, float* g_uncert, float* g_density, const float* const* terms, const float* weights, int n,
                             float* out, const int32_t* mlp_status, int32_t* bad, int n_bad, int word_status, int word_finite,
                             int32_t* snapshot, uint64_t* step_counter, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K9  InstanceNorm2d (affine = False) + LeakyReLU of the PatchGAN ladder, one launch per derivative order
 * ref: layers/discriminator.py:94-115 (IN(c) + LeakyReLU(0.2) after each stride-2 SN-conv);
 *      the double backward serves the R1 penalty, model/nerf_adapt_st_gan.py:794-807 (compute_grad2).
 * x, y, xhat, gy, gx, ggx: [n_inst, hw] (n_inst = images x channels, hw = H*W), rstd: [n_inst].
 * ------------------------------------------------------------------------------------------ */
int tp_inorm_lrelu_fwd(const float* x, int64_t n_inst, int hw, float eps, float slope, float* y, float* xhat, float* rstd,
                       tp_stream_t stream);
/* addend (optional, [n_inst, hw]): a second cotangent of x that is added to the result (the R1 path's, K16) */
int tp_inorm_lrelu_bwd(const float* xhat, const float* rstd, const float* gy, int64_t n_inst, int hw, float slope,
                       const float* addend, float* gx, tp_stream_t stream);
/* cotangent ggx of gx -> gradients wrt gy and wrt x (through xhat and rstd) */
int tp_inorm_lrelu_bwd_bwd(const float* xhat, const float* rstd, const float* gy, const float* ggx, int64_t n_inst, int hw,
                           float slope, float* g_gy, float* g_x, tp_stream_t stream);

/* ---- pairs: TWO independent problems of one kernel in ONE launch (workgroups [0, n_a) work on the first, the rest on the second).  The
 * discriminator step (reference model/nerf_adapt_st_gan.py:129-171) passes the real and the fake patch stack through the same ladder and
 * tail one after the other; both passes' launches are latency-sized at these shapes (10-15 us for a few hundred kFLOP..MFLOP), so a pair
 * takes the time of one.  The two problems must not share an output, a split-K workspace, tile counters or a ticket. */
typedef struct tp_inorm_bwd_args {
  const float* xhat; const float* rstd; const float* gy;
  int64_t n_inst; int32_t hw; float slope;
  const float* addend;     /* or NULL */
  float* gx;
} tp_inorm_bwd_args;
int tp_inorm_lrelu_bwd_pair(const tp_inorm_bwd_args* a, const tp_inorm_bwd_args* b, tp_stream_t stream);


/* ------------------------------------------------------------------------------------------
 * K10  RMSprop step of the PatchGAN parameters in one launch (reference optim_disc.step(),
 * model/nerf_adapt_st_gan.py:168, torch.optim.RMSprop: alpha 0.99, eps 1e-8, no momentum / centring / weight decay).
 * lr_dev != NULL: the learning rate is read from device memory (a hipGraph-captured step); else lr_host.
 * ------------------------------------------------------------------------------------------ */
#define TP_RMSPROP_MAX_TENSORS 16
typedef struct tp_rmsprop_tensor {
  float* param;            /* [numel] updated in place */
  const float* grad;       /* [numel] */
  float* square_avg;       /* [numel] updated in place */
  int64_t numel;
  float* step;             /* optional 0-dim float device tensor (torch's state "step"): += 1 by the same launch when the step is applied */
} tp_rmsprop_tensor;
/* gate: n_gate int32 device words (or 0): if any is non-zero the launch changes nothing (a flagged step, see tp_step_flags) */
/* hyper-parameters as doubles: 1 - alpha is formed in double and then rounded, like torch's scalar arithmetic */
int tp_rmsprop_step(const tp_rmsprop_tensor* tensors /* host array */, int n, const float* lr_dev, double lr_host, double alpha,
                    double eps, const int32_t* gate, int n_gate, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K11  The stride-2 4x4 convolutions of the PatchGAN ladder (reference layers/discriminator.py:94-115:
 *      Conv2d(c_in, c_out, (4,4), (2,2), (1,1), bias=False) under spectral_norm, called through
 *      model/nerf_adapt_st_gan.py:129-171 and differentiated twice by compute_grad2, :794-807).  Three implicit-GEMM
 *      kernels on the fp32 matrix cores, closed under differentiation (a convolution is bilinear in input and weight):
 *        tp_conv4s2_fwd    out = y  [N,Co,H/2,W/2] = conv(x, w)
 *        tp_conv4s2_dgrad  out = gx [N,C,H,W]      = conv_transpose(gy, w)     (every element written)
 *        tp_conv4s2_wgrad  out = gw [Co,C,4,4]     = sum over images and positions of gy (x) window(x)
 *      Dense fp32 NCHW / OIHW tensors; H, W powers of two >= 8.  `workspace` holds split-K partial sums
 *      (tp_conv4s2_workspace floats, may be NULL when that is 0), `counters` one zero-initialised uint32 per output
 *      tile (n_counters of tp_conv4s2_workspace; the kernels leave them zero).  Fixed summation order: deterministic.
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_conv4s2_args {
  const float* x;          /* [N,C,H,W]        fwd, wgrad */
  const float* w;          /* [Co,C,4,4]       fwd, dgrad */
  const float* gy;         /* [N,Co,H/2,W/2]   dgrad, wgrad */
  float* out;
  float* workspace;
  void* counters;
  int32_t N, C, H, W, Co;
  /* dgrad, optional (in_gx != NULL; H = W = 8): the InstanceNorm + LeakyReLU backward of the ladder stage in FRONT of this convolution
   * (tp_inorm_lrelu_bwd with gy = this data gradient: xhat [N,C,8,8], rstd [N*C], addend or NULL, gx = in_gx) inside the same launch,
   * bit-identical to the two launches; skip_out != 0: the data gradient itself is not written (out may then be NULL... it is not read) */
  int32_t skip_out;
  const float* in_xhat; const float* in_rstd; const float* in_addend; float* in_gx;
  float in_slope; int32_t pad_;
  /* tp_conv4s2_fwd_inorm[_pair], optional: the launch also copies x to x_copy (16-byte aligned, N C H W a multiple of 4) */
  float* x_copy;
} tp_conv4s2_args;
#define TP_CONV_FWD 0
#define TP_CONV_DGRAD 1
#define TP_CONV_WGRAD 2
/* floats of workspace the operation `op` (TP_CONV_*) needs for these sizes; *n_counters = number of uint32 counters */
int64_t tp_conv4s2_workspace(const tp_conv4s2_args* args, int op, int64_t* n_counters);
int tp_conv4s2_fwd(const tp_conv4s2_args* args, tp_stream_t stream);
/* The forward convolution with the InstanceNorm2d (affine = False) + LeakyReLU that follows it in the ladder in ONE launch, for 4x4 and
 * 8x8 output maps (reference layers/discriminator.py:94-115): out = y = lrelu(xhat), xhat [N,Co,H/2,W/2], rstd [N*Co] as
 * tp_inorm_lrelu_fwd returns them; the convolution's own output is not materialised.  Workspace / counters:
 * tp_conv4s2_fwd_inorm_workspace (-1: map size not covered -> two launches). */
int64_t tp_conv4s2_fwd_inorm_workspace(const tp_conv4s2_args* args, int64_t* n_counters);
int tp_conv4s2_fwd_inorm(const tp_conv4s2_args* args, float eps, float slope, float* xhat, float* rstd, tp_stream_t stream);
int tp_conv4s2_dgrad(const tp_conv4s2_args* args, tp_stream_t stream);
int tp_conv4s2_wgrad(const tp_conv4s2_args* args, tp_stream_t stream);
int tp_conv4s2_fwd_inorm_pair(const tp_conv4s2_args* a, float* xhat_a, float* rstd_a, const tp_conv4s2_args* b, float* xhat_b, float* rstd_b,
                              float eps, float slope, tp_stream_t stream);            /* same map size in both problems */
int tp_conv4s2_dgrad_pair(const tp_conv4s2_args* a, const tp_conv4s2_args* b, tp_stream_t stream);
int tp_conv4s2_wgrad_pair(const tp_conv4s2_args* a, const tp_conv4s2_args* b, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K12  3x3 / stride 1 / padding 1 convolution (+ bias, + ReLU) of the frozen perceptual-loss feature network
 *      (reference layers/perceptual_loss.py:8-45, torchvision VGG19 features[:15]; model/nerf_adapt_st_gan.py:758-766).
 *        tp_conv3s1_fwd    out [N,Co,H,W] = relu?(conv(inp [N,C,H,W], w [Co,C,3,3]) + bias)
 *        tp_conv3s1_dgrad  out [N,C,H,W]  = conv_transpose(inp [N,Co,H,W] * (mask > 0), w)    (mask = the forward output of a
 *                          ReLU layer, or NULL)
 *      H, W powers of two >= 4.  Workspace / counters as for K11 (tp_conv3s1_workspace, op TP_CONV_FWD / TP_CONV_DGRAD).
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_conv3s1_args {
  const float* inp;
  const float* w;
  const float* bias;       /* fwd: [Co] or NULL */
  const float* mask;       /* dgrad: [N,Co,H,W] or NULL */
  float* out;
  float* workspace;
  void* counters;
  int32_t N, C, H, W, Co;
  int32_t relu;            /* fwd: apply max(., 0) */
} tp_conv3s1_args;
int64_t tp_conv3s1_workspace(const tp_conv3s1_args* args, int op, int64_t* n_counters);
int tp_conv3s1_fwd(const tp_conv3s1_args* args, tp_stream_t stream);
int tp_conv3s1_dgrad(const tp_conv3s1_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K13  Small per-iteration pieces of the training step, one launch each (csrc/train_misc.hip)
 * ------------------------------------------------------------------------------------------ */
/* FlexPatchSampler.__call__ (reference tools/patch_sampler.py:80-114).  u [3,B] uniforms (scale, x shift,
 * y shift), lattice [p] = linspace(-1, 1, p); the annealed lower scale bound from device memory (lo_dev, a captured step)
 * or from the host (lo_host, span_host = (float)(hi - lo) formed in double like the reference's Python arithmetic).
 * coords [B,p,p,2] in grid_sample (x, y) order, scales [B].
 * u == NULL: the uniforms are drawn inside the kernel -- Philox4x32-10, key = seed, counter (b, c_lo, 'patc', c_hi) with c = *counter
 * (a device word: the step counter of a captured training step; NULL = 0), words x, y, z -> scale, x shift, y shift of image b. */
int tp_patch_coords(const float* u, int B, int p, const float* lattice, const float* lo_dev, float lo_host, float span_host,
                    float hi, int random_scale, int random_shift, uint64_t seed, const uint64_t* counter, float* coords, float* scales,
                    tp_stream_t stream);
/* mean binary_cross_entropy_with_logits(x [n], target) for a constant target (compute_gan_loss 'standard',
 * model/nerf_adapt_st_gan.py:809-823): out [1]; backward gx [n] = g[0] (sigmoid(x) - target) / n. */
int tp_bce_logits_fwd(const float* x, int n, float target, float* out, tp_stream_t stream);
int tp_bce_logits_bwd(const float* x, int n, float target, const float* g, float* gx, tp_stream_t stream);
/* The four image batches of the feature loss (model/nerf_adapt_st_gan.py:758-766), ImageNet-normalised
 * (layers/perceptual_loss.py:19-20): out [4B,3,P] = [rgb | rgb m + image (1-m) | image m + image_syn pad | image],
 * pad = (mask_syn == 1 and m == 0); backward: g_rgb [B,P,3] from g_out [4B,3,P] (only the first 2B images count). */
typedef struct tp_feat_inputs_args {
  const float* rgb;        /* [B,P,3] rendered colours */
  const float* gathered;   /* [B,n_channels,P] tp_patch_gather output */
  int32_t B, P, n_channels;
  int32_t c_image, c_image_syn, c_mask, c_mask_syn;   /* first channel of each in `gathered` */
  float mean[3], std[3];
} tp_feat_inputs_args;
int tp_feat_inputs_fwd(const tp_feat_inputs_args* args, float* out, tp_stream_t stream);
int tp_feat_inputs_bwd(const tp_feat_inputs_args* args, const float* g_out, float* g_rgb, tp_stream_t stream);
/* K18 -- the whole feature-loss chain of the generator step in ONE call (17 launches): the four image stacks (tp_feat_inputs_fwd), the
 * frozen feature network F = torchvision VGG19 features[:15] (reference layers/perceptual_loss.py:8-45: 3x3 convolutions 3-64, 64-64,
 * max pool, 64-128, 128-128, max pool, 128-256, 256-256, 256-256, ReLU after each but the last), the two-pair loss
 * model/nerf_adapt_st_gan.py:758-766   loss = mse(F(fake1), F(real1)) + w2 mse(F(fake2), F(real2))   (targets detached)
 * and its gradient wrt the rendered colours: g_rgb = scale * d loss / d rgb.  Pools, ReLU derivatives and un-pooling ride in the
 * convolutions' epilogues; only the 2B fake images are differentiated.  16 x 16 patches (the reference's patch_size).
 * loss[3] = {l1 + w2 l2, l1, l2}.  workspace / counters: sizes from tp_feat_chain_workspace; the counters must be zero before the first
 * call and are left zero; both belong to ONE stream (calls that may overlap on different streams need their own). */
#define TP_FEAT_CHAIN_LAYERS 7
typedef struct tp_feat_chain_args {
  const float* rgb;        /* [B,P,3] rendered colours, P = H * W */
  const float* gathered;   /* [B,n_channels,P] tp_patch_gather output */
  int32_t B, H, W, n_channels;
  int32_t c_image, c_image_syn, c_mask, c_mask_syn;   /* first channel of each in `gathered` */
  float mean[3], std[3];                               /* ImageNet normalisation constants */
  const float* packed;                                 /* the seven [Co,C,3,3] weights as tp_feat_chain_pack wrote them */
  const float* bias[TP_FEAT_CHAIN_LAYERS];             /* [Co] */
  float w2;                /* weight of the second pair (the reference: 5) */
  float scale;             /* cotangent of the loss (the caller's loss weight 10^w; 1 for the plain gradient) */
  float* loss;             /* [3] */
  float* g_rgb;            /* [B,P,3] */
  float* workspace; int64_t workspace_floats;
  int32_t* counters; int64_t n_counters;
} tp_feat_chain_args;
int64_t tp_feat_chain_workspace(int32_t B, int32_t H, int32_t W, int64_t* n_counters);   /* floats; -1: shape not covered */
/* The frozen weights in the kernels' operand order, once per set of weights: packed [tp_feat_chain_packed_floats()] = for every layer
 * [C][9][Co] (forward) followed by, for every layer, [Co][9, taps flipped][C] (data gradient) -- a half-wavefront's 32 produced channels
 * are 128 consecutive bytes.  w: host array of the seven [Co,C,3,3] device tensors. */
int64_t tp_feat_chain_packed_floats(void);
int tp_feat_chain_pack(const float* const* w, float* packed, tp_stream_t stream);
int tp_feat_chain(const tp_feat_chain_args* args, tp_stream_t stream);
/* The discriminator step's inputs (model/nerf_adapt_st_gan.py:478-497, no gradient): real [B,nc,P] = image m + rgb pad,
 * fake [B,nc,P] = rgb, nc = 3 or (geo) 9 with the masked nocs / normal channels 6..11 of `gathered` [B,14,P] appended. */
/* Step gate of a captured training step (the reference asserts every weighted loss term finite on the host,
 * model/base.py:153-154): bad[word_status] |= mlp_status[0] & 1 (mlp_status may be NULL), bad[word_finite] |= !isfinite(total[0]),
 * then snapshot[0..n_bad) = bad[0..n_bad) -- the words the optimiser launch of this step reads as its gate. */
int tp_step_flags(const int32_t* mlp_status, const float* total, int32_t* bad, int n_bad, int word_status, int word_finite,
                  int32_t* snapshot, tp_stream_t stream);
/* torch.optim.Adam step (reference optim_nerf, model/nerf_adapt_st_gan.py:62-68,125; no weight decay, no amsgrad) for up to
 * TP_ADAM_MAX_TENSORS tensors in one launch; `step` = 0-dim float tensor holding the steps taken so far (the block that finishes last
 * launch adds 1 to each afterwards); learning rate from device memory (lr_dev) or the host; gate as for tp_rmsprop_step.
 * ticket: ONE zero-filled device word owned by the calling stream (arrival counter of the block that advances the step counters;
 * the launch leaves it zero); launches that may overlap on different streams of a device need different words. */
#define TP_ADAM_MAX_TENSORS 32
typedef struct tp_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* step;
  int64_t numel;
} tp_adam_tensor;
int tp_adam_step(const tp_adam_tensor* tensors /* host array */, int n, const float* lr_dev, double lr_host, double beta1, double beta2,
                 double eps, const int32_t* gate, int n_gate, uint32_t* ticket, tp_stream_t stream);
/* The per-iteration host -> device state of a replayed training step (reference Model.train_iteration's move_to_device of the
 * batch, model/nerf_adapt_st_gan.py:212; patch_sampler.iterations :185; discriminator.progress :182) in ONE launch:
 * n_copies contiguous device-to-device copies (16-byte aligned; the batch into the captured step's static inputs),
 * n_scalars host values written to device floats, and n_words int32 gate words copied out to device-visible pinned host memory
 * (words_dst may be NULL). */
#define TP_STEP_INPUTS_MAX_COPIES 24
#define TP_STEP_INPUTS_MAX_SCALARS 8
typedef struct tp_step_copy { void* dst; const void* src; int64_t bytes; } tp_step_copy;
int tp_step_inputs(const tp_step_copy* copies /* host array */, int n_copies, float* const* scalar_dst /* host array */,
                   const float* scalar_val /* host array */, int n_scalars, const int32_t* words_src, int32_t* words_dst, int n_words,
                   tp_stream_t stream);
/* Data parallel (no reference counterpart: options.py:112 asserts a single GPU; BASELINE.json config C4): the gradients of ONE
 * optimiser step into the flat fp32 buffer that one RCCL all-reduce sums -- flat[concatenation of the n tensors] = scale * grads[k]
 * (grads[k] NULL: zeros; scale = 1 / world, so the sum is the average) -- and the step-gate words into the buffer's tail as 0 / 1 floats:
 * tail[j] = (words[j] != 0 || tail[j] != 0) for j < n_words (words may be NULL).  The tail is STICKY: after the all-reduce it is
 * non-zero on every rank if any rank set it, in this or an earlier step, and read as int32 words it is the gate tp_adam_step /
 * tp_rmsprop_step take.  One launch. */
#define TP_GRAD_PACK_MAX_TENSORS 32
int tp_grad_pack(const float* const* grads /* host array */, const int64_t* numel /* host array */, int n, float* flat, float scale,
                 const int32_t* words, int n_words, float* tail, tp_stream_t stream);
/* Diagnostic (no reference counterpart): number of nodes (kernel launches, fills, copies) recorded so far in the hipGraph that `stream`
 * is capturing into, -1 when it is not capturing (the launch counts of a captured training iteration). */
int64_t tp_capture_node_count(tp_stream_t stream);
/* Diagnostic (no reference counterpart): the device's 100 MHz constant clock written to *slot by a one-thread launch in stream order. */
int tp_stamp(uint64_t* slot, tp_stream_t stream);
/* Diagnostic (no reference counterpart): one sleeping wave samples the shader clock against the 100 MHz constant clock over `windows`
 * consecutive windows of window_us microseconds: out[2w] = shader cycles, out[2w+1] = 100-MHz ticks of window w (out: 2 * windows device
 * words).  Launched on a side stream in front of a kernel, it reports the clock the chip holds under that kernel's load. */
int tp_clock_probe(uint64_t* out, int windows, int64_t window_us, tp_stream_t stream);
int tp_disc_inputs(const float* rgb, const float* gathered, int B, int P, int geo, float* real, float* fake, tp_stream_t stream);
/* Cotangent of the fake stack wrt the rendered colours (the nerf step back-propagates D(fake) into the render):
 * g_rgb [B,P,3] = g_fake [B,nc,P] channels 0..2, transposed. */
int tp_fake_patch_bwd(const float* g_fake, int B, int P, int nc, float* g_rgb, tp_stream_t stream);
/* Feature loss of the generator step (model/nerf_adapt_st_gan.py:762-766; layers/perceptual_loss.py:39-45): feat [4n] = network
 * features of [fake1 | fake2 | real1 | real2] (n floats each); out3 = {l1 + w2 l2, l1, l2} with l_i = mean((fake_i - real_i)^2);
 * backward g_feat [4n] for the cotangent g[0] of out3[0] (targets detached: their quarters are zero). */
int tp_feat_pair_loss_fwd(const float* feat, int64_t n, float w2, float* out3, tp_stream_t stream);
int tp_feat_pair_loss_bwd(const float* feat, int64_t n, float w2, const float* g, float* g_feat, tp_stream_t stream);
/* R1 penalty value (model/nerf_adapt_st_gan.py:794-807 and the mean over the batch its caller takes, :149): out[0] = sum(g^2) / B
 * for g [B,m] (n = B m floats); backward out [n] = 2 g cot[0] / B. */
int tp_sumsq_mean_fwd(const float* g, int64_t n, int B, float* out, tp_stream_t stream);
int tp_sumsq_mean_bwd(const float* g, int64_t n, int B, const float* cot, float* out, tp_stream_t stream);
/* K16 (the discriminator step as an explicit schedule): value and weighted gradient of the R1 penalty in one launch,
 * out[0] = sum(g^2) / B, out[1] = w out[0] (what the reference logs), out_g [n] = 2 w g / B (w = the term's loss weight, a host
 * constant);
 * and both GAN-loss terms of the discriminator step (model/nerf_adapt_st_gan.py:139-160) with their weighted cotangents:
 * out2 = {bce(d_real, 1), bce(d_fake, 0)}, g_real [n] = w_real (sigmoid(d_real) - 1) / n, g_fake [n] = w_fake sigmoid(d_fake) / n. */
int tp_sumsq_mean_fwd_bwd(const float* g, int64_t n, int B, float w, float* out, float* out_g, tp_stream_t stream);
/* MaxPool2d(2, 2) of the feature network (layers/perceptual_loss.py:8-18): x [n, H, W] (n = images x channels; H, W even) ->
 * y [n, H/2, W/2], arg [n, H/2, W/2] = position 0..3 of the maximum inside its window (the first one on ties, NaN wins: torch's
 * rule); backward gx [n, H, W] from gy and arg, every element written (no zero fill). */
int tp_maxpool2_fwd(const float* x, int64_t n, int H, int W, float* y, uint8_t* arg, tp_stream_t stream);
int tp_maxpool2_bwd(const float* gy, const uint8_t* arg, int64_t n, int H, int W, float* gx, tp_stream_t stream);
int tp_gan_disc_losses(const float* d_real, const float* d_fake, int n, float w_real, float w_fake, float* out2, float* g_real,
                       float* g_fake, tp_stream_t stream);
/* Rows idx[b] of the two latent tables (model/nerf_adapt_st_gan.py:589-593) in one launch, and the dense table gradients
 * gw [n_rows,C] = sum over b with idx[b] == r of g[b] (ascending b; every element written: no zero-fill needed). */
/* out[0] = sum_k weights[k] * terms[k][0] (ascending k) for up to 16 scalar device tensors; `terms` and `weights` are HOST
 * arrays (the weighted loss total of model/base.py:145-157, for logging and the step gate). */
int tp_weighted_sum(const float* const* terms, const float* weights, int n, float* out, tp_stream_t stream);
/* the same followed by tp_step_flags on the result, in one launch (the captured training step: loss total + step gate) */
int tp_weighted_sum_flags(const float* const* terms, const float* weights, int n, float* out, const int32_t* mlp_status, int32_t* bad,
                          int n_bad, int word_status, int word_finite, int32_t* snapshot, uint64_t* step_counter /* optional: += 1 */,
                          tp_stream_t stream);
/* idx_copy (optional, [B]): the launch also copies idx there -- the backward of a captured step reads that private copy, so that the
 * caller's idx buffer may be refilled for the next iteration while this one's backward is still to run */
int tp_latent_rows_fwd(const float* w_trans, const float* w_light, const int64_t* idx, int B, int C_trans, int C_light, float* out_trans,
                       float* out_light, int64_t* idx_copy, tp_stream_t stream);
int tp_latent_rows_bwd(const float* g_trans, const float* g_light, const int64_t* idx, int B, int n_rows, int C_trans, int C_light,
                       float* gw_trans, float* gw_light, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K14  Scale-conditioned head of the PatchGAN (reference layers/discriminator.py:30-40,112-115):
 *      a = [z, sin(s 2^l pi), cos(s 2^l pi) (l < L), s];  out = W3 lrelu(W2 lrelu(W1 lrelu(a)))   (1x1 SN-convs, no bias)
 *      one launch each for the forward, the backward (gz, gW1..3) and the R1 double backward (cotangent c_gz of gz ->
 *      d/d g_out and d/d W1..3; model/nerf_adapt_st_gan.py:794-807).  t0 [B,Cin] / t1 / t2 [B,H] are the saved activations
 *      (Cin = C + 2L + 1), e1 / e2 [B,H] the backward's intermediates the double backward re-uses.
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_disc_head_args {
  const float* z;          /* [B,C]   fwd */
  const float* scale;      /* [B]     fwd */
  const float* W1;         /* [H,Cin] */
  const float* W2;         /* [H,H] */
  const float* W3;         /* [H] */
  const float* g_out;      /* [B]     bwd, bwd_bwd */
  const float* c_gz;       /* [B,C]   bwd_bwd */
  float* t0; float* t1; float* t2;   /* fwd: written; bwd, bwd_bwd: read */
  float* e1; float* e2;              /* bwd: written; bwd_bwd: read */
  float* out;              /* fwd: [B];  bwd: gz [B,C];  bwd_bwd: d/d g_out [B] */
  float* gW1; float* gW2; float* gW3;   /* bwd, bwd_bwd: [H,Cin], [H,H], [H]; bwd: all three NULL = data gradient only */
  int32_t B, C, L, H;
  float slope;
  int32_t accumulate_gw;   /* bwd: gW1..3 += (after the double backward wrote its share there) */
} tp_disc_head_args;
int tp_disc_head_fwd(const tp_disc_head_args* args, tp_stream_t stream);
int tp_disc_head_bwd(const tp_disc_head_args* args, tp_stream_t stream);
int tp_disc_head_bwd_bwd(const tp_disc_head_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K15  y = x W^T for a handful of rows: the PatchGAN's last ladder convolution covers its whole map (reference
 *      layers/discriminator.py:110-111), i.e. [B, 8192] x [8192, 64] with B = 4 .. 32.  Forward and weight gradient
 *      (gW = gy^T x) and data gradient gx = gy W (kernel for M <= 16, a library GEMM beyond).  x [M,K], w [N,K], y [M,N].
 * ------------------------------------------------------------------------------------------ */
int tp_skinny_linear_fwd(const float* x, const float* w, float* y, int M, int N, int K, tp_stream_t stream);
int tp_skinny_linear_wgrad(const float* gy, const float* x, float* gw, int M, int N, int K, tp_stream_t stream);
/* gx [M,K] = gy [M,N] w [N,K] for M <= 16 rows (larger M: a library GEMM on the host side) */
int tp_skinny_linear_dgrad(const float* gy, const float* w, float* gx, int M, int N, int K, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K17  the TAIL of the PatchGAN = K15's full-map convolution + K14's scale-conditioned head in ONE launch per derivative order
 *      (reference layers/discriminator.py:30-40,110-115; the R1 double backward of model/nerf_adapt_st_gan.py:794-807).
 *      Up to TP_DISC_TAIL_MAX_ROWS rows per pass; N = C = ndf, Cin = N + 2 L + 1, K a multiple of 4.
 *      fwd:      a [M,K], W0 [N,K], scale [M], W1..3 -> out [M], t0 [M,Cin], t1, t2 [M,H]
 *      bwd:      g_out [M], t0..2, W0..3 -> (all optional) gz [M,N], e1, e2 [M,H], c_a [M,K] = gz W0, gW0 [N,K] = sum_rows gz (x) a
 *                (+ sum over M2 extra rows gy2 [M2,N] (x) a2 [M2,K]: the R1 path's pair of the same weight), gW1..3 (all or none;
 *                accumulate_gw adds to what is there)
 *      bwd_bwd:  a = c [M,K] (cotangent of the first pass' c_a), g_out, t0..2, e1, e2, W0..3 -> gW1..3 (the double backward's
 *                share), out = d/d g_out [M] (optional)
 *      workspace: tp_disc_tail_workspace_bytes(N) bytes; ticket: one zero-filled device word owned by the calling stream (fwd, bwd_bwd).
 * ------------------------------------------------------------------------------------------ */
#define TP_DISC_TAIL_MAX_ROWS 16
typedef struct tp_disc_tail_args {
  const float* a;          /* fwd: ladder output [M,K]; bwd: the same (for gW0; may be NULL without gW0); bwd_bwd: c [M,K] */
  const float* W0;         /* [N,K] */
  const float* scale;      /* [M]   fwd */
  const float* W1; const float* W2; const float* W3;   /* [H,Cin], [H,H], [H] */
  const float* g_out;      /* [M]   bwd, bwd_bwd */
  float* t0; float* t1; float* t2;   /* fwd: written; bwd, bwd_bwd: read */
  float* e1; float* e2;              /* bwd: written (optional); bwd_bwd: read */
  float* out;              /* fwd: [M]; bwd_bwd: d/d g_out [M] (optional) */
  float* gz;               /* bwd: [M,N] (optional) */
  float* c_a;              /* bwd: [M,K] (optional) */
  float* gW0;              /* bwd: [N,K] (optional) */
  const float* gy2;        /* bwd: [M2,N] extra cotangent rows of gW0 */
  const float* a2;         /* bwd: [M2,K] their inputs */
  float* gW1; float* gW2; float* gW3;
  /* bwd, optional: the InstanceNorm2d + LeakyReLU backward of the ladder's LAST stage (K9 tp_inorm_lrelu_bwd) applied to c_a inside the
   * launch: c_z [M,K] = rstd P(c_a s(xhat)) (+ in_addend); an instance = in_P consecutive columns (in_P | 64: the 4x4 map's 16),
   * xhat [M,K], rstd [M K / in_P].  c_a may then be NULL (only c_z is written). */
  const float* in_xhat; const float* in_rstd; const float* in_addend; float* c_z; int32_t in_P;
  void* workspace;         /* fwd, bwd_bwd */
  uint32_t* ticket;        /* fwd, bwd_bwd */
  int32_t M, M2, K, N, L, H;
  float slope;
  int32_t accumulate_gw;
} tp_disc_tail_args;
size_t tp_disc_tail_workspace_bytes(int N);
int tp_disc_tail_fwd(const tp_disc_tail_args* args, tp_stream_t stream);
int tp_disc_tail_bwd(const tp_disc_tail_args* args, tp_stream_t stream);
int tp_disc_tail_bwd_bwd(const tp_disc_tail_args* args, tp_stream_t stream);
int tp_disc_tail_fwd_pair(const tp_disc_tail_args* a, const tp_disc_tail_args* b, tp_stream_t stream);
int tp_disc_tail_bwd_pair(const tp_disc_tail_args* a, const tp_disc_tail_args* b, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K19  hard mesh rasteriser for the surfel maps of the adaptation loops (rgbsyn_<loop>, nocs_<loop>, normal_<loop>)
 * ref: compute_surfelinfo.py:37-56,100-140, tools/mvrenderer.py:33-180,695-730 (PyTorch3D, faces_per_pixel = 1),
 *      compute_box.py:41-60.  One face per pixel: the minimum of (view-space z, face index), so the result does not
 *      depend on the order faces are visited in.  OpenCV pinhole: x_c = R X + t, (u, v) = (K x_c)[:2] / (K x_c)[2];
 *      pixel (row i, column j) is sampled at (j + 0.5, i + 0.5); covered iff all three barycentrics are > 0 (either
 *      winding); degenerate faces and faces with a vertex at z <= 0 are dropped.  Background: zbuf = -1, face = -1,
 *      rgb = nocs = normal = 0.  rgb / nocs: perspective-correct interpolation of vcolor / of the vertices normalised as
 *      ((v - nocs_center) / nocs_scale + 1) / 2.  normal: compute_surfelinfo.normal_from_depth of zbuf (object frame,
 *      third component negated, border and zbuf <= 0 zero).  Three launches; every output except zbuf may be NULL.
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_mesh_raster_args {
  const float* verts;      /* [V,3] object frame, mm */
  const int32_t* faces;    /* [F,3] vertex indices (out-of-range indices drop the face) */
  const float* vcolor;     /* [V,3] in [0,1]; may be NULL when rgb is NULL */
  float nocs_center[3];    /* host values: per-axis vertex mean */
  float nocs_scale[3];     /* host values: per-axis max |v - mean| (> 0 when nocs is requested) */
  const float* pose;       /* [B,3,4] [R|t] object -> camera, t in mm */
  const float* intr;       /* [B,3,3] */
  int B, H, W, V, F;
  int normals_from_zbuf;   /* non-zero: only the normal stage runs, on zbuf as given (an input); verts / faces / V / F unused */
  float* zbuf;             /* [B,H,W] out: view-space z in mm, -1 on background */
  int32_t* face;           /* [B,H,W] out or NULL: face index, -1 on background */
  float* rgb;              /* [B,H,W,3] out or NULL */
  float* nocs;             /* [B,H,W,3] out or NULL */
  float* normal;           /* [B,H,W,3] out or NULL */
  void* workspace;         /* tp_mesh_raster_workspace_bytes(B, H, W, F) bytes, 16-byte aligned */
} tp_mesh_raster_args;
size_t tp_mesh_raster_workspace_bytes(int B, int H, int W, int F);
int tp_mesh_raster(const tp_mesh_raster_args* args, tp_stream_t stream);
/* K34  tp_mesh_raster with the face chunks culled per tile: the same arguments, refusals and limits, and every output plane is
 *      tp_mesh_raster's bit for bit for every input (any face order, dropped faces, NaN poses, a mesh outside the image;
 *      normals_from_zbuf runs the normal stage alone, as there).  One launch more (four, three without normals): after the face
 *      setup one int4 per (image, chunk of 256 face records) takes the union of the chunk's pixel boxes, and a 16 x 16 tile
 *      enters a chunk only if that box overlaps it.  A pixel keeps the minimum of (bits of z, face index) over the faces shown to
 *      it, and a skipped chunk holds no face whose box reaches the tile, so the minimum is unchanged.  The gain depends on how
 *      compact the chunks are on screen: a face order that is coherent in space (texpose_amd.surfel.coherent_face_order) gives the
 *      most, a shuffled one still skips every tile outside the object's box.
 *      workspace: 64 B F bytes of face records, then 16 bytes per (image, chunk): 64 B F + 16 B ceil(F / 256), 16-byte aligned;
 *      the query returns 0 for B <= 0 or F <= 0.  No allocation, no host synchronisation, no atomics; safe to capture. */
size_t tp_mesh_raster_culled_workspace_bytes(int B, int H, int W, int F);
int tp_mesh_raster_culled(const tp_mesh_raster_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K20  the data layer's finish of the surfel maps: from tp_mesh_raster's outputs to the four tensors the reference's data
 *      layer hands the trainer (image_syn, mask_syn, nocs_pred, normal_pred), without the files in between.
 * ref: data/lm.py:196-253 (get_predicted_synthetic_image / get_predicted_nocs / get_predicted_normal),
 *      data/lm.py:497-521 (get_edge, smooth_geo), compute_surfelinfo.py:118-140 (the 8-bit encode of the PNG files).
 *      q(x) = float(uint8(trunc(x *_f32 255))) /_f32 255 (one fp32 product, truncation toward zero, the correctly rounded fp32
 *      quotient).  The integer is clamped to [0, 255]: numpy's float -> uint8 cast is undefined outside that range, and the
 *      rasteriser cannot produce such values (interpolated colours / NOCS lie in [0, 1] up to rounding); NaN gives 0.
 *      image_syn = q(rgb) (zero when rgb is NULL), mask_syn = zbuf > 0 ? 1 : 0, nocs_pred = smooth_geo(q(nocs)),
 *      normal_pred = smooth_geo(normal) (the .npz is float32: no quantisation).  smooth_geo: the mask is channel 0 != 0 of
 *      the map being smoothed (after q for NOCS); an edge pixel is in the mask and has a 4-neighbour inside the image that
 *      is not; its three channels become the medians of the 3x3 neighbourhood of the unsmoothed map with replicated
 *      borders (cv2.medianBlur(x, 3)); every other pixel keeps its value.  quantize = 0 skips q for rgb and nocs (not what
 *      the reference trains on; for callers who do not want the 8-bit loss).
 *      One launch; inputs interleaved [B,H,W,3], outputs planar [B,3,H,W]; outputs must not overlap inputs (a pixel reads
 *      its neighbours).  Every output may be NULL.  Safe to capture.
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_surfel_finish_args {
  const float* rgb;        /* [B,H,W,3] or NULL (mesh without vertex colours: image_syn = 0) */
  const float* nocs;       /* [B,H,W,3]; may be NULL when nocs_pred is NULL */
  const float* normal;     /* [B,H,W,3]; may be NULL when normal_pred is NULL */
  const float* zbuf;       /* [B,H,W], <= 0 on background */
  int B, H, W;
  int quantize;            /* non-zero: the 8-bit round trip q on rgb and nocs (the reference's files) */
  float* image_syn;        /* [B,3,H,W] out or NULL */
  float* mask_syn;         /* [B,H,W] out or NULL */
  float* nocs_pred;        /* [B,3,H,W] out or NULL */
  float* normal_pred;      /* [B,3,H,W] out or NULL */
} tp_surfel_finish_args;
int tp_surfel_finish(const tp_surfel_finish_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K21  scene depth bounds, object labels and blended mesh depth for novel views: the z-buffer blend of K objects at B poses.
 * ref: model/nerf_pretrain.py:307-416 (nerf_pretrain_env.py carries the same code): per object a slab test of its box against
 *      every pixel ray (camera.py:292-314,415-433) and a depth render of its mesh; torch.where / min / gather / where over the
 *      stack; data/lm.py:352-356 (range_source 'render': 0.8 x and 1.2 x the depth).
 *      Per pixel, with z_k = zbuf_k > 0 ? zbuf_k : 100000 (mm; NaN counts as background):
 *        winner  = the lowest k with the smallest z_k;  covered = zbuf_winner > 0
 *        depth   = covered ? (z_winner /_f32 1000) *_f32 depth_scale : 0
 *        label   = covered ? ids[winner] : 0
 *        TP_SCENE_BOX    : label > 0 ? (t_near, t_far) of the winner's box on the pixel ray where the slab test is valid
 *                          (t_far > 0 && t_far > t_near), (0, 0) where it is not : (bg_near, bg_far).  The ray is tp_raygen's
 *                          TP_PIX_INDEX ray of the pixel (centre (j + 0.5, i + 0.5)), the slab test is tp_aabb's: the same device
 *                          functions.  Unlike TP_BOUNDS_AABB, a non-positive t_near (camera inside the box) is kept.
 *        TP_SCENE_RENDER : covered ? (depth *_f32 0.8f, depth *_f32 1.2f) : (bg_near, bg_far)
 *        TP_SCENE_NONE   : (bg_near, bg_far); label and depth are still written.
 *      Every operation is one rounded fp32 step (correctly rounded division, no fused multiply-add).
 *      One launch, no workspace; outputs must not overlap inputs.  Safe to capture.
 * ------------------------------------------------------------------------------------------ */
#define TP_SCENE_MAX_OBJECTS 32
enum tp_scene_source {   /* options nerf.depth.range_source */
  TP_SCENE_BOX = 0,
  TP_SCENE_RENDER = 1,
  TP_SCENE_NONE = 2
};
typedef struct tp_scene_bounds_args {
  const float* pose;       /* [B,3,4] [R|t] object -> camera, t in NeRF units (depth_scale per metre); TP_SCENE_BOX only, else may be NULL */
  const float* intr;       /* [B,3,3]; TP_SCENE_BOX only, else may be NULL */
  const float* zbuf;       /* [K,B,H,W] tp_mesh_raster's zbuf of every object: view-space z in mm, <= 0 on background */
  const float* boxes;      /* [K,2,3] device: (min, max) of every object's box in NeRF units (bb_mm * depth_scale / 1000);
                            * TP_SCENE_BOX only, else may be NULL */
  const int32_t* ids;      /* [K] device: the label of every object (> 0) */
  int B, H, W;
  int K;                   /* 1 .. TP_SCENE_MAX_OBJECTS */
  int source;              /* tp_scene_source */
  float depth_scale;       /* NeRF units per metre (options nerf.depth.scale) */
  float bg_near, bg_far;   /* the background range, NeRF units (nerf.depth.range * nerf.depth.scale) */
  float* z_near;           /* [B,H*W] out */
  float* z_far;            /* [B,H*W] out */
  int32_t* label;          /* [B,H*W] out */
  float* depth;            /* [B,H*W] out: NeRF units, 0 where uncovered */
} tp_scene_bounds_args;
int tp_scene_bounds(const tp_scene_bounds_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K22  the per-object annotations a BOP scene folder stores for a frame (scene_gt_info.json, mask/, mask_visib/), for K objects
 *      at B poses, from K21's inputs and output; and the 8-bit / 16-bit images of a rendered view (rgb/, depth/).
 * ref: data/lm.py:161-180,255-300 (what the reference's data layer reads of such a folder); the rules themselves are the BOP
 *      format's, restated in tests/scene_annotate_ref.py.
 *      tp_scene_annotate, per object k, pose b, pixel p (x = column, y = row):
 *        all_k(p)   = zbuf[k,b,p] > 0                      (NaN counts as background)
 *        visib_k(p) = all_k(p) && label[b,p] == ids[k]     (ids must be distinct)
 *        info[b,k]  = { px_count_all, px_count_visib, xmin, ymin, xmax, ymax of all_k, xmin, ymin, xmax, ymax of visib_k }:
 *                     inclusive pixel indices; an empty set gives -1 in its four extents
 *        mask[b,k,p] = all_k(p) ? 255 : 0,  mask_visib[b,k,p] = visib_k(p) ? 255 : 0
 *      The call initialises info itself (a first launch writes 0 / -1, the second accumulates with integer atomics: add, signed
 *      max, unsigned min): no memset by the caller, no workspace, no allocation, no host synchronisation; integer reductions, so
 *      the result is exactly reproducible.  Outputs must not overlap inputs.  Safe to capture.
 *      tp_view_images, one rounded fp32 operation per step, NaN -> 0:
 *        rgb8    = uint8(trunc(clamp(rgb, 0, 1) *_f32 255))
 *        depth16 = uint16(trunc(clamp((depth /_f32 depth_scale) *_f32 png_per_metre, 0, 65535)))
 *      One launch.  Either pair (rgb, rgb8) / (depth, depth16) may be NULL as a whole.  Safe to capture.
 * ------------------------------------------------------------------------------------------ */
#define TP_SCENE_INFO_FIELDS 10
typedef struct tp_scene_annotate_args {
  const float* zbuf;       /* [K,B,H,W] tp_mesh_raster's zbuf of every object: view-space z in mm, <= 0 or NaN on background */
  const int32_t* label;    /* [B,H*W] tp_scene_bounds' label: the id of the nearest object, 0 where nothing is covered */
  const int32_t* ids;      /* [K] device: the label of every object, distinct */
  int B, H, W;
  int K;                   /* 1 .. TP_SCENE_MAX_OBJECTS */
  int32_t* info;           /* [B,K,TP_SCENE_INFO_FIELDS] out */
  uint8_t* mask;           /* [B,K,H,W] out or NULL: 0 / 255 */
  uint8_t* mask_visib;     /* [B,K,H,W] out or NULL: 0 / 255 */
} tp_scene_annotate_args;
int tp_scene_annotate(const tp_scene_annotate_args* args, tp_stream_t stream);

typedef struct tp_view_images_args {
  const float* rgb;        /* [B,H*W,3] or NULL */
  const float* depth;      /* [B,H*W] in NeRF units (depth_scale per metre), or NULL */
  int B, H, W;
  float depth_scale;       /* NeRF units per metre (options nerf.depth.scale) */
  float png_per_metre;     /* depth16 units per metre (2000: the file stores half millimetres) */
  uint8_t* rgb8;           /* [B,H,W,3] out (NULL with rgb) */
  uint16_t* depth16;       /* [B,H,W] out (NULL with depth) */
} tp_view_images_args;
int tp_view_images(const tp_view_images_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K23  Lab chroma loss of the generator step (loss_weight.lab) and its gradient wrt the rendered colours, one launch each way.
 * ref: model/nerf_adapt_st_gan.py:772-773, layers/lab_loss.py:13-48; the colour conversion is kornia.color.rgb_to_lab as
 *      published, restated in tests/lab_ref.py, not pinned to a kornia call.
 *      Per pixel, fake = rgb, real = the three planes at `real`:  lab(c) = normalize_lab(rgb_to_lab(c)),
 *        l = SmoothL1(lab(fake)[1] - lab(real)[1]) + SmoothL1(lab(fake)[2] - lab(real)[2])      (beta = 1, the two chroma channels)
 *        mask given:  sums = { sum l * mask, sum mask },   loss = sums[0] / sums[1]      (no epsilon: an empty mask gives NaN)
 *        mask NULL:   sums = { sum l, 2 * B * P },         loss = sums[0] / sums[1]      (the mean over both channels)
 *        fake_lab = lab(fake) with its L plane replaced by lab(real)'s, real_lab = lab(real)
 *      fp32 in and out; each value is the rule evaluated in fp64 registers and rounded once.  The sums are reduced per wavefront,
 *      per block and by the last block to arrive over the blocks in ascending order, all in double: no float atomics, the result
 *      does not depend on the order the blocks ran in.  The backward recomputes the Lab values from the inputs and reads sums[1];
 *      it writes every element of g_rgb.  No allocation, no host synchronisation; outputs must not overlap inputs.  Safe to capture.
 * ------------------------------------------------------------------------------------------ */
#define TP_LAB_LOSS_MAX_BLOCKS 256
typedef struct tp_lab_loss_args {
  const float* rgb;             /* [B,P,3]  the rendered colours (composite output) */
  const float* real;            /* channel c of image b, pixel p: real[b * real_batch_stride + c * real_channel_stride + p] --
                                   channels 3..5 of tp_patch_gather's [B,14,P] (strides 14 P, P) or a dense [B,3,P] (3 P, P) */
  const float* mask;            /* pixel p of image b: mask[b * mask_batch_stride + p], or NULL */
  int64_t real_batch_stride, real_channel_stride, mask_batch_stride;      /* in floats */
  int B, P;
  float* fake_lab;              /* fwd, optional [B,3,P] */
  float* real_lab;              /* fwd, optional [B,3,P] */
  void* workspace;              /* fwd: 2 * TP_LAB_LOSS_MAX_BLOCKS doubles */
  double* sums;                 /* [2]  (fwd: out, bwd: in) */
  float* loss;                  /* fwd: [1] */
  uint32_t* ticket;             /* fwd: ONE zero-filled device word owned by the calling stream (tp_nerf_losses_args.ticket's rules); the
                                   launch leaves it zero.  Unused by the backward. */
} tp_lab_loss_args;
int tp_lab_loss_fwd(const tp_lab_loss_args* args, tp_stream_t stream);
/* g: the upstream gradient of the loss, one device scalar; g_rgb [B,P,3] = g[0] * d loss / d rgb */
int tp_lab_loss_bwd(const tp_lab_loss_args* args, const float* g, float* g_rgb, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K24  brute-force 1-nearest / 1-farthest neighbour in 3-D: the search under ADD-S, the model diameter and the one-directional
 *      chamfer distance (texpose_amd/pose_error.py; the definitions are restated in tests/pose_error_ref.py).
 * ref: camera.py:469-586 (p2p_distance: PyTorch3D's knn_points with K = 1).
 *      Per batch element b and query i < x_len[b], with bx = (Bx == 1 ? 0 : b), bt = (Bt == 1 ? 0 : b), the distance is taken
 *      between q = x[bx,i] and the targets y' = y[bt,j], j < y_len[bt]; or, with A, between A[b][:, :3] x[bx,i] + A[b][:, 3] and
 *      y[bt,j], evaluated in the frame before A's translation t = A[b][:, 3]: q = A[b][:, :3] x[bx,i] (in fp64, rounded once to
 *      fp32) and y' = y[bt,j] -_f32 t.  Both sides are then of the model's size rather than of the camera distance, where fp32
 *      roundings are ~1e-5 mm instead of ~1e-4 mm.  The mapped cloud is never stored; with Bx = 1 one model is searched under B maps.
 *        d2(j) = dx*dx + dy*dy + dz*dz of the fp32 differences q - y'   (the direct form; dx*dx rounded, then two fused
 *                multiply-adds -- one fixed evaluation order)
 *        TP_NN1_NEAREST : the smallest d2(j), TP_NN1_FARTHEST : the largest; on equal d2 the LOWEST j wins
 *        a target with a NaN coordinate never wins (nor any j whose d2 is NaN)
 *        no winner (NaN query, i >= x_len[b], no target left): d2 = +inf (-inf in TP_NN1_FARTHEST), idx = -1
 *      The result is a function of the inputs alone: where the targets are split over workgroups (target_slices), the slices meet
 *      through a 64-bit integer key (bits of d2, then index) and integer atomic min / max -- no float atomics; the call writes the
 *      keys' initial value itself.  One launch without slices, three with.  No allocation, no host synchronisation; outputs and
 *      workspace must not overlap inputs.  Safe to capture.
 * ------------------------------------------------------------------------------------------ */
#define TP_NN1_TILE 1024                /* targets staged in LDS at a time */
#define TP_NN1_QUERIES_PER_BLOCK 1024   /* queries one workgroup owns (256 threads x 4) */
enum tp_nn1_mode {
  TP_NN1_NEAREST = 0,
  TP_NN1_FARTHEST = 1
};
typedef struct tp_nn1_args {
  const float* x;          /* [Bx,P1,3] queries */
  const float* y;          /* [Bt,P2,3] targets */
  const int32_t* x_len;    /* [B] or NULL (= P1 everywhere); clamped to 0 .. P1 */
  const int32_t* y_len;    /* [Bt] or NULL (= P2 everywhere); clamped to 0 .. P2 */
  const float* A;          /* [B,3,4] or NULL: the affine map applied to the queries of b */
  int B;                   /* batch elements: rows of A, of x_len and of the outputs */
  int Bx, Bt;              /* 1 (one query set / one target set shared by every b) or B */
  int P1, P2;
  int mode;                /* tp_nn1_mode */
  int target_slices;       /* 0: chosen from the shapes; n > 0: min(n, number of target tiles) slices.  The result does not depend on it */
  float* d2;               /* [B,P1] out */
  int32_t* idx;            /* [B,P1] out */
  void* workspace;         /* tp_nn1_workspace_bytes(args) bytes (0: may be NULL); needs no clearing */
} tp_nn1_args;
/* B * P1 * 8 where the call splits the targets into more than one slice, else 0 (and 0 for arguments tp_nn1 refuses) */
size_t tp_nn1_workspace_bytes(const tp_nn1_args* args);
int tp_nn1(const tp_nn1_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K25  the per-pose errors of the BOP evaluation that need no search: ADD, MSSD, MSPD and the mean projection error, for B pose
 *      pairs over one model and its S symmetry transforms.  The BOP definitions are restated (tests/pose_error_ref.py), not pinned
 *      to a bop_toolkit call.  With e = P_e x, g_s = P_g S_s x and pi(X) = (fx X / Z + cx, fy Y / Z + cy):
 *        out[b] = { add  = mean_x |e - g_0|,              mssd = min_s max_x |e - g_s|,
 *                   mspd = min_s max_x |pi(e) - pi(g_s)|,  proj = mean_x |pi(e) - pi(g_0)| }
 *        s_mssd[b], s_mspd[b]: the winning s, the lowest on ties
 *      sym[0] must be the identity (add and proj are taken at s = 0).  mspd, proj and s_mspd are written only when intr is given.
 *      A point with Z <= 0 (or NaN) under P_e or any P_g S_s makes mspd = proj = NaN and s_mspd = -1 for that b; add and mssd are
 *      unaffected.  fp32 in and out, fp64 in between, reduced by a fixed tree (one workgroup per (b, s), then the minimum over s in
 *      a second launch): bit-identical from run to run.  S > TP_POSE_ERRORS_MAX_SYM is refused (-1, tp_last_error).
 *      Two launches.  No allocation, no host synchronisation; outputs must not overlap inputs.  Safe to capture.
 * ------------------------------------------------------------------------------------------ */
#define TP_POSE_ERRORS_MAX_SYM 64
typedef struct tp_pose_errors_args {
  const float* pts;        /* [M,3] model points */
  const float* pose_est;   /* [B,3,4] */
  const float* pose_gt;    /* [B,3,4] */
  const float* sym;        /* [S,3,4], row 0 the identity */
  const float* intr;       /* [B,3,3] or NULL */
  int M, B, S;
  float* out;              /* [B,4]: add, mssd, mspd, proj (columns 2, 3 untouched without intr) */
  int32_t* s_mssd;         /* [B] */
  int32_t* s_mspd;         /* [B]; may be NULL without intr */
  void* workspace;         /* B * S * 4 doubles; needs no clearing */
} tp_pose_errors_args;
int tp_pose_errors(const tp_pose_errors_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K26  the per-pixel part of BOP's Visible Surface Discrepancy (VSD, cost 'step', visibility 'bop19') for B pose pairs and T
 *      misalignment tolerances (texpose_amd/pose_error.py; restated in tests/vsd_ref.py, not pinned to a bop_toolkit call; DESIGN
 *      section 16).  Per pose pair b, with K = intr[b], the test plane d = depth_test[frame ? frame[b] : (Ft == 1 ? 0 : b)] and, at
 *      the pixel in row i and column j,
 *        f        = sqrt(((j + 0.5 - cx) / fx)^2 + ((i + 0.5 - cy) / fy)^2 + 1)      (the project's pixel centres, not the toolkit's (j, i))
 *        D_x      = z_x * f for x in {est, gt, test}: the distance from the camera centre
 *        ok(z)    = z > 0                              (a NaN is not ok)
 *        missing  = !(d > 0)                           (0, negative, NaN; the toolkit tests == 0)
 *        vis(z)   = ok(z) && (missing || D_z - D_test <= delta_mm)
 *        V_gt     = vis(z_gt),   V_est = vis(z_est) || (V_gt && ok(z_est))
 *        I = V_gt && V_est,      U = V_gt || V_est
 *        n_U = |U|, n_I = |I|, c_t = |{p in I : |D_gt - D_est| >= tau_mm[b,t]}|
 *        err[b,t] = (c_t + n_U - n_I) / n_U, and 1 where n_U = 0
 *      Everything between the fp32 inputs and the integer counts is fp64, evaluated as written (left to right, no contraction); err
 *      is the fp64 quotient rounded once.  The counts meet through integer atomic adds only, so the outputs are a function of the
 *      inputs alone: bit-identical from run to run and under graph replay.  The call clears counts itself.  A frame[b] outside
 *      [0, Ft) is the caller's error; it is CLAMPED into the range, nothing is read out of bounds.  T outside 1 .. TP_VSD_MAX_TAUS,
 *      non-positive sizes, H * W >= 2^31 and, without frame, an Ft that is neither 1 nor B are refused (-1, tp_last_error).
 *      Three launches.  No allocation, no host synchronisation; outputs must not overlap inputs.  Safe to capture.
 * ------------------------------------------------------------------------------------------ */
#define TP_VSD_MAX_TAUS 16
typedef struct tp_vsd_args {
  const float* z_est;        /* [B,H,W] mm, <= 0 or NaN: background */
  const float* z_gt;         /* [B,H,W] */
  const float* depth_test;   /* [Ft,H,W] mm, 0: no measurement */
  const int32_t* frame;      /* [B] index into depth_test, or NULL: b when Ft == B, 0 when Ft == 1 */
  const float* intr;         /* [B,3,3] */
  const float* tau_mm;       /* [B,T] */
  float delta_mm;
  int B, Ft, H, W, T;        /* 1 <= T <= TP_VSD_MAX_TAUS (16) */
  int32_t* counts;           /* [B, 2+T] out: n_U, n_I, c_0 .. c_{T-1}; the caller clears nothing */
  float* err;                /* [B,T] out */
} tp_vsd_args;
int tp_vsd(const tp_vsd_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K27  bake B posed images onto the V vertices of a mesh as weighted colour sums (texpose_amd/texture_bake.py; restated in
 *      tests/texture_bake_ref.py; the project's own step, no reference code).  Per vertex i and view b, in
 *      ascending b, with [R|t] = pose[b], K = intr[b], v = verts[i], n = normals[i]:
 *        x      = R v + t,  z = x_z;                      the pair is skipped unless z > 0
 *        c      = -(((R n) . x) / |x|);                    skipped unless c >= cos_min          (no image memory is touched so far)
 *        q      = K x,  (u, v) = (q_0, q_1) / q_2;        pixel (row r, column j) has its centre at (j + 0.5, r + 0.5)
 *        su = u - 0.5, sv = v - 0.5, j0 = floor(su), r0 = floor(sv), a = su - j0, be = sv - r0
 *        taps (r0 + dr, j0 + dj), dr, dj in {0, 1}, with weights w = (dj ? a : 1 - a) * (dr ? be : 1 - be)
 *        tol    = z_tol_mm + slope * (z / min(K_00, K_11)) * sqrt(max(0, 1 - c * c)) / c
 *                 (the depth a plane of that obliquity gains over the <= sqrt(2) px to a tap: a shadow-map bias from the normal)
 *        a tap is valid iff it lies inside the image, zbuf_tap > 0, |zbuf_tap - z| <= tol, and its three colour channels (and
 *                 its weight sample, if weight is given) are finite
 *        cover  = sum of w over the valid taps (in the order (0,0), (0,1), (1,0), (1,1) of (dr, dj));  skipped unless cover >= cover_min
 *        colour = (sum of w * rgb_tap over the valid taps) / cover
 *        wb     = c * cover, times (sum of w * weight_tap over the valid taps) / cover if weight is given
 *        acc[i] += wb * (colour_r, colour_g, colour_b, 1),  count[i] += 1
 *      A pair whose (su, sv) is not inside [-1, W) x [-1, H) (a NaN included) has no tap inside the image and is skipped before
 *      anything is read.  Everything between the fp32 inputs and a pair's four products is fp64, evaluated as written (left to
 *      right, no contraction).  The views are cut into S = ceil(B / L) slices of L = max(4, ceil(B / ceil(65536 / V))) consecutive
 *      views (at most B): S depends on V and B alone, never on the device.  One thread per (vertex, slice) adds its pairs in
 *      ascending b in fp64 and stores the partial sums into the workspace; a second launch adds a vertex's S partial sums in
 *      ascending order in fp64 and writes acc = fl32(sum) where clear is non-zero, acc = fl32(fp64(acc) + sum) otherwise, and the
 *      same for count.  No atomics: the outputs are a function of the inputs alone, bit-identical from run to run, from device
 *      to device and under graph replay.  Non-positive sizes, B > 65535, H * W >= 2^31, V > 2^30, cos_min or cover_min
 *      outside (0, 1] and a negative or NaN z_tol_mm or slope are refused (-1, tp_last_error).  Nothing is read out of
 *      bounds for any pose.  Two launches.  No allocation, no host synchronisation; outputs and workspace must not overlap inputs.
 *      Safe to capture.
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_texture_bake_args {
  const float* verts;        /* [V,3] model frame, mm */
  const float* normals;      /* [V,3] unit, model frame */
  const float* pose;         /* [B,3,4] [R|t] model -> camera, t in mm (K19's convention) */
  const float* intr;         /* [B,3,3] */
  const float* rgb;          /* [B,H,W,3] */
  const float* zbuf;         /* [B,H,W] K19's plane: mm, <= 0 or NaN: background */
  const float* weight;       /* [B,H,W] or NULL */
  int V, B, H, W;
  int clear;                 /* non-zero: acc and count are overwritten; zero: added to */
  float cos_min, cover_min, z_tol_mm, slope;
  float* acc;                /* [V,4] in/out: sum of wb * r, wb * g, wb * b, wb */
  int32_t* count;            /* [V] in/out: contributing views */
  void* workspace;           /* tp_texture_bake_workspace_bytes(V, B) bytes, 16-byte aligned; needs no clearing */
} tp_texture_bake_args;
int tp_texture_bake_slices(int V, int B);                 /* S of the rule above; 0 for non-positive sizes */
size_t tp_texture_bake_workspace_bytes(int V, int B);
int tp_texture_bake(const tp_texture_bake_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K28  batched PnP-RANSAC: poses from dense 2D-3D correspondence (NOCS) maps (texpose_amd/pnp.py; restated in tests/pnp_ref.py; the
 *      project's own step, no reference code).  Common inputs: xy [B,N,2] pixel coordinates (pixel (row r,
 *      column j) has its centre at (j + 0.5, r + 0.5)), xyz [B,N,3] model points in mm, count [B] (image b uses the entries
 *      0 .. n-1 with n = count[b] CLAMPED into [0, N]), intr [B,3,3] (fx = K_00, fy = K_11, cx = K_02, cy = K_12; no skew), poses
 *      [R|t] model -> camera in mm, row-major 12 floats.  Every call launches on the caller's stream, allocates nothing and never
 *      synchronises; all of them are safe to capture.  No input value (NaN, Inf, huge poses, a count outside [0, N]) causes an access
 *      out of bounds.  Non-positive B, N, T or stride, T > TP_PNP_MAX_HYP, a tau_px that is not finite and positive, iters outside
 *      0 .. TP_PNP_MAX_ITERS, H * W >= 2^31 and null pointers are refused (-1, tp_last_error) before anything is launched.
 *
 *      tp_corr_from_nocs: the strided pixels k = 0 .. N-1, N = ceil(H / stride) * ceil(W / stride), (r, j) = (k / Ws * stride,
 *      k % Ws * stride) with Ws = ceil(W / stride), are visited in ascending k (= ascending r * W + j).  A pixel is kept iff its
 *      mask is non-zero (uint8, or float with mask_is_float; a NaN is non-zero) and its three NOCS values q are finite; the kept
 *      ones are written densely in that order as xy = (j + 0.5, r + 0.5), xyz_c = (2 q_c - 1) * scale_c + centre_c in fp32 as
 *      written (no contraction), and count[b] is their number.  Entries from count[b] on are not written.  Ranks come from wave
 *      ballots, per-tile counts (256 pixels) and their prefix sums: no atomic cursor, the order is a function of the inputs alone.
 *      Two launches.
 *
 *      tp_pnp_hypotheses: hypothesis h of image b draws w = philox4x32_10(counter (b, h, 0x706E7034 'pnp4', 0), key (seed low,
 *      seed high)) and from it four distinct indices: i0 = mulhi(w0, n), i1 = mulhi(w1, n-1), i2 = mulhi(w2, n-2), i3 = mulhi(w3,
 *      n-3), each of i1, i2, i3 moved past the earlier ones (visited in ascending order: i += 1 for every earlier index <= i);
 *      sample_idx = (i0, i1, i2, i3), or four -1 where n < 4.  In fp64: the bearings f_k = normalise((u - cx) / fx, (v - cy) / fy,
 *      1) of the first three, the P3P quartic in v = s3 / s1 (Grunert's elimination: s2 = u s1, 2 u (cos g - v cos a) =
 *      (k-1) v^2 - 2 k cos b v + 1 + k with k = (a^2 - c^2) / b^2), its real roots in closed form (Ferrari) with two Newton steps
 *      each, per root with v > 0, u > 0 the depths, polished by two Newton steps on the three distance equations themselves (the
 *      quartic's coefficients cancel where two roots are close), and [R|t] as the rigid motion between the two triangles from their
 *      orthonormal frames.  The kept solution has the smallest squared reprojection error on the fourth point (infinite where its depth is not
 *      positive; ties go to the smaller v).  hyp_valid = 0, and hyp is 12 zeros, when n < 4, a sampled value is not finite, the
 *      three image points are collinear (twice the triangle's area <= 1e-9 x the sum of two squared edges), there is no real root,
 *      no root has three positive depths, or the pose is not finite.  One thread per hypothesis.
 *
 *      tp_pnp_score: inliers[b,h] = the number of entries i < n with, in fp32 as written (no contraction),
 *        x = ((R_k0 X + R_k1 Y) + R_k2 Z) + t_k,  x_z > 0 and finite,
 *        du = ((fx * x_x) / x_z + cx) - u,  dv = ((fy * x_y) / x_z + cy) - v,  du * du + dv * dv <= tau_px * tau_px
 *      (a NaN anywhere fails the comparison).  valid (or NULL: all valid): a hypothesis with valid = 0 counts 0.  A workgroup holds
 *      1024 points of one image in registers and walks all T poses (the pose index is uniform: the 12 floats come through scalar
 *      loads, the valid bytes of 64 poses as one ballot); per pose a wave ballot and popcount, LDS integer sums across the waves,
 *      one integer atomic add per (workgroup, pose) to inliers, which the call clears itself: integer sums do not depend on the
 *      order of arrival.  With inlier_mask [B,N] given, a further launch writes inlier_mask[b,i] = 1 where entry i is an inlier of
 *      pose sel[b], 0 elsewhere (i >= n, an invalid pose, a sel outside [0, T) and a NULL sel included); it is a launch of its own
 *      because a byte store inside the pose loop would take the pose loads off the scalar unit.  Two launches, three with the mask.
 *
 *      tp_pnp_refine: the winner of image b is the valid hypothesis with the largest hyp_inliers, the lowest h among equals.  Then
 *      iters Gauss-Newton steps in fp64 throughout (the fp32 inputs widened; the inlier test as above but in fp64).  Each step is a
 *      reduce launch (ceil(N / 1024) workgroups per image, a function of N alone: the inliers of the current pose at tau, for them
 *      the 21 + 6 entries of J^T J and J^T r, sum |r|^2 and the count, for x' = x + w x x + v in the camera frame, parameters (w, v);
 *      butterfly sums inside a wave, the four waves in ascending order) and a solve launch per image (the partials in ascending
 *      order; keep-best: the pose just evaluated replaces the stored best iff its count is higher, or equal at a lower sum |r|^2;
 *      then J^T J is factored by Cholesky: a pivot that is not finite or <= 1e-10 x its diagonal entry means NOT POSITIVE DEFINITE:
 *      status 3, the best pose so far is kept and nothing more changes; otherwise (J^T J + 1e-3 diag(J^T J)) d = -J^T r is solved
 *      by Cholesky, R <- exp(w) R, t <- exp(w) t + v with Rodrigues' formula, and R is re-orthonormalised (Gram-Schmidt on its first
 *      two columns, the third their cross product)).  One more reduce and compare evaluates the last iterate.  pose [B,3,4] = the
 *      best pose rounded to fp32, inliers its count, rms = sqrt(sum |r|^2 / count) in px (NaN at count 0), status 0 = ok, 1 = n < 4,
 *      2 = no valid hypothesis, 3 as above; with status 1 or 2 pose and rms are NaN and inliers is 0.  The returned count is never
 *      below the winner's own count under the same fp64 test.  3 + 2 iters launches.
 * ------------------------------------------------------------------------------------------ */
#define TP_PNP_MAX_HYP 4096
#define TP_PNP_MAX_ITERS 32
typedef struct tp_corr_from_nocs_args {
  const float* nocs;         /* [B,H,W,3] */
  const void* mask;          /* [B,H,W] uint8, or float where mask_is_float is non-zero */
  int mask_is_float;
  float centre[3], scale[3]; /* surfel.nocs_normalisation: a vertex v maps to ((v - centre) / scale + 1) / 2 */
  int B, H, W, stride;
  float* xy;                 /* [B,N,2] out, N = ceil(H / stride) * ceil(W / stride) */
  float* xyz;                /* [B,N,3] out */
  int32_t* count;            /* [B] out */
  void* workspace;           /* tp_pnp_workspace_bytes(B, N, 1) bytes; needs no clearing */
} tp_corr_from_nocs_args;
typedef struct tp_pnp_hypotheses_args {
  const float* xy;           /* [B,N,2] */
  const float* xyz;          /* [B,N,3] */
  const int32_t* count;      /* [B] */
  const float* intr;         /* [B,3,3] */
  int B, N, T;
  uint64_t seed;
  int32_t* sample_idx;       /* [B,T,4] out */
  float* hyp;                /* [B,T,12] out */
  uint8_t* hyp_valid;        /* [B,T] out */
} tp_pnp_hypotheses_args;
typedef struct tp_pnp_score_args {
  const float* xy;
  const float* xyz;
  const int32_t* count;
  const float* intr;
  const float* poses;        /* [B,T,12] */
  const uint8_t* valid;      /* [B,T] or NULL */
  int B, N, T;
  float tau_px;
  int32_t* inliers;          /* [B,T] out; the caller clears nothing */
  const int32_t* sel;        /* [B] or NULL: the pose whose inliers inlier_mask marks */
  uint8_t* inlier_mask;      /* [B,N] out, or NULL */
} tp_pnp_score_args;
typedef struct tp_pnp_refine_args {
  const float* xy;
  const float* xyz;
  const int32_t* count;
  const float* intr;
  const float* hyp;          /* [B,T,12] */
  const uint8_t* hyp_valid;  /* [B,T] or NULL */
  const int32_t* hyp_inliers;/* [B,T] */
  int B, N, T;
  float tau_px;
  int iters;                 /* 0 .. TP_PNP_MAX_ITERS */
  float* pose;               /* [B,3,4] out */
  int32_t* inliers;          /* [B] out */
  float* rms;                /* [B] out */
  int32_t* status;           /* [B] out */
  void* workspace;           /* tp_pnp_workspace_bytes(B, N, T) bytes, 16-byte aligned; needs no clearing */
} tp_pnp_refine_args;
size_t tp_pnp_workspace_bytes(int B, int N, int T);       /* 0 for non-positive sizes */
int tp_corr_from_nocs(const tp_corr_from_nocs_args* args, tp_stream_t stream);
int tp_pnp_hypotheses(const tp_pnp_hypotheses_args* args, tp_stream_t stream);
int tp_pnp_score(const tp_pnp_score_args* args, tp_stream_t stream);
int tp_pnp_refine(const tp_pnp_refine_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K29  one step of batched projective point-to-plane ICP: B poses refined against measured depth (texpose_amd/icp.py; restated in
 *      tests/icp_ref.py; the project's own step, no reference code).  zbuf / face are K19's planes of the mesh
 *      rendered at pose; the call compares them with the measured depth and takes one damped Gauss-Newton step of the update
 *      x' = x + w x x + v in the camera frame (parameters (w, v), as tp_pnp_refine).  Per pixel (row i, column j) of image b, with
 *      K = intr[b] (fx = K_00, fy = K_11, cx = K_02, cy = K_12), [R|t] = pose[b] and the depth plane fr = frame ? frame[b] CLAMPED
 *      into [0, Ft) : (Ft == 1 ? 0 : b), everything in fp64 from the fp32 inputs, evaluated as written (no contraction):
 *        1. z = zbuf[b,i,j];           skipped unless z > 0 and finite
 *        2. f = face[b,i,j];           skipped unless 0 <= f < F and the three vertex indices of faces[f] lie in [0, V)
 *        3. d = depth[fr,i,j];         skipped unless d > 0 and finite, and where mask is given and mask[fr,i,j] == 0
 *        4. ray = ((j + 0.5 - cx) / fx, (i + 0.5 - cy) / fy, 1),  q = (ray_x^2 + ray_y^2) + 1,  P = z ray,  Q = d ray;
 *           kept iff ((d - z) * (d - z)) * q <= tau_mm * tau_mm          (a NaN fails)
 *        5. m = R ((v1 - v0) x (v2 - v0)), each row ((R_k0 c_x + R_k1 c_y) + R_k2 c_z);  skipped unless |m|^2 is finite and > 0;
 *           n = m * (1 / sqrt(|m|^2)), negated where n . ray > 0: the face's own flat normal, towards the camera
 *        6. r = n . (P - Q),  J = [P x n, n]
 *      and the 29 sums of tp_pnp_refine over the kept pixels: the 21 upper-triangle entries of J^T J (row-major), the 6 of J^T r,
 *      sum r^2 and the count.  A thread owns four consecutive flat pixels (ascending), a workgroup 1024; butterfly sums inside a
 *      wave, the four waves in ascending order, one record per workgroup, the records in ascending order: no atomics, the outputs
 *      are a function of the inputs alone, bit-identical from run to run and under graph replay.  Per image:
 *        inliers = count;  rms = sqrt(sum r^2 / count) in mm (NaN at count 0): both describe `pose`, the pose the planes show
 *        status  = 1 where count < 6; else 3 where J^T J is NOT POSITIVE DEFINITE by tp_pnp_refine's pivot rule (a Cholesky pivot
 *                  that is not finite or <= 1e-10 x its diagonal entry), or, without evaluate_only, where the damped matrix does
 *                  not factor or the stepped pose is not finite in fp32; else 0
 *        pose_out = (status == 0 and not evaluate_only): (J^T J + damping diag(J^T J)) delta = -J^T r solved by Cholesky,
 *                  R <- exp(w) R, t <- exp(w) t + v with Rodrigues' formula, Gram-Schmidt on R's first two columns (the third
 *                  their cross product), rounded to fp32;  otherwise pose, bit for bit (pose_out may be NULL with evaluate_only)
 *      Status is an output only: a failed step passes its pose through, so a loop over steps needs no state.  Non-positive sizes,
 *      B > 65535, H * W >= 2^31, without frame an Ft that is neither 1 nor B, a tau_mm that is not finite and positive, a damping
 *      that is not finite and >= 0, null pointers, a workspace that is not 16-byte aligned and pose_out == pose are refused (-1,
 *      tp_last_error) before anything is launched.  No input value (NaN, Inf, a face or vertex index out of range, huge poses)
 *      causes an access out of bounds.  Two launches.  No allocation, no host synchronisation; outputs and workspace must not
 *      overlap inputs.  Safe to capture.
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_depth_icp_args {
  const float* verts;        /* [V,3] model frame, mm */
  const int32_t* faces;      /* [F,3] */
  const float* zbuf;         /* [B,H,W] K19's depth of the mesh at pose: mm, <= 0 or NaN: background */
  const int32_t* face;       /* [B,H,W] K19's face index, -1: background */
  const float* pose;         /* [B,3,4] the pose zbuf and face were rendered at */
  const float* intr;         /* [B,3,3] */
  const float* depth;        /* [Ft,H,W] measured depth in mm; <= 0, NaN, Inf: no measurement */
  const int32_t* frame;      /* [B] index into depth (and mask), or NULL: b when Ft == B, 0 when Ft == 1 */
  const uint8_t* mask;       /* [Ft,H,W] or NULL; 0: the pixel is skipped */
  int V, F, B, Ft, H, W;
  float tau_mm;              /* finite, > 0: the largest distance along the ray between model and measurement of a kept pixel */
  float damping;             /* finite, >= 0: relative Levenberg damping of the diagonal */
  int evaluate_only;         /* non-zero: inliers, rms and status of pose; no step */
  float* pose_out;           /* [B,3,4] out; may be NULL with evaluate_only; must not be pose */
  int32_t* inliers;          /* [B] out */
  float* rms;                /* [B] out, mm */
  int32_t* status;           /* [B] out: 0 ok, 1 fewer than 6 kept pixels, 3 not positive definite */
  void* workspace;           /* tp_depth_icp_workspace_bytes(B, H, W) bytes, 16-byte aligned; needs no clearing */
} tp_depth_icp_args;
size_t tp_depth_icp_workspace_bytes(int B, int H, int W);  /* 256 * B * ceil(H * W / 1024), rounded up to 16; 0 for non-positive sizes */
int tp_depth_icp_step(const tp_depth_icp_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K30  one step of batched photometric alignment: B poses refined against a photograph (texpose_amd/photo_align.py; restated in
 *      tests/photo_ref.py; the project's own step, no reference code).  zbuf / rgb are K19's planes of the
 *      vertex-coloured mesh rendered at pose; the call compares rgb with the photograph and takes one damped Gauss-Newton step of
 *      the update x' = x + w x x + v in the camera frame (parameters (w, v), as tp_depth_icp_step): a surface point keeps its
 *      colour, the pixel it lands on moves, and the photograph's own central-difference gradient says what it would see there.
 *      Per pixel (row i, column j) of image b, with K = intr[b] (fx = K_00, fy = K_11, cx = K_02, cy = K_12) and the photograph
 *      fr = frame ? frame[b] CLAMPED into [0, Ft) : (Ft == 1 ? 0 : b), everything in fp64 from the fp32 inputs, evaluated as
 *      written (no contraction):
 *        1. skipped unless 1 <= i <= H - 2 and 1 <= j <= W - 2 (an image with H < 3 or W < 3 keeps nothing)
 *        2. z = zbuf[b,i,j];           skipped unless z > 0 and finite
 *        3. skipped where mask is given and mask[fr,i,j] == 0
 *        4. c_k = rgb[b,i,j,k], o_k = image[fr,i,j,k] and the four neighbours image[fr,i,j-1,k], image[fr,i,j+1,k],
 *           image[fr,i-1,j,k], image[fr,i+1,j,k] for k = 0, 1, 2;  skipped unless all 18 values are finite
 *        5. r_k = o_k - c_k;  kept iff (r_0^2 + r_1^2) + r_2^2 <= tau * tau          (a NaN fails)
 *        6. gx_k = 0.5 (image[fr,i,j+1,k] - image[fr,i,j-1,k]),  gy_k = 0.5 (image[fr,i+1,j,k] - image[fr,i-1,j,k]),
 *           rx = ((j + 0.5) - cx) / fx,  ry = ((i + 0.5) - cy) / fy,  P = (z rx, z ry, z),
 *           a_k = (gx_k fx / z,  gy_k fy / z,  -((gx_k fx) rx + (gy_k fy) ry) / z),  J_k = [P x a_k, a_k]
 *      and the 29 sums of tp_pnp_refine, accumulated over the three rows (J_k, r_k) of a kept pixel in channel order: the 21
 *      upper-triangle entries of J^T J (row-major), the 6 of J^T r, sum r_k^2 and the count, + 1 per kept PIXEL.  A thread owns
 *      four consecutive flat pixels (ascending), a workgroup 1024; butterfly sums inside a wave, the four waves in ascending
 *      order, one record per workgroup, the records in ascending order: no atomics, the outputs are a function of the inputs
 *      alone, bit-identical from run to run and under graph replay.  Per image:
 *        inliers = count;  rms = sqrt(sum r_k^2 / count) in colour units (NaN at count 0): both describe `pose`
 *        status  = 1 where count < 6; else 3 where J^T J is NOT POSITIVE DEFINITE by tp_pnp_refine's pivot rule (a Cholesky pivot
 *                  that is not finite or <= 1e-10 x its diagonal entry), or, without evaluate_only, where the damped matrix does
 *                  not factor or the stepped pose is not finite in fp32; else 0
 *        pose_out = (status == 0 and not evaluate_only): (J^T J + damping diag(J^T J)) delta = -J^T r solved by Cholesky,
 *                  R <- exp(w) R, t <- exp(w) t + v with Rodrigues' formula, Gram-Schmidt on R's first two columns (the third
 *                  their cross product), rounded to fp32;  otherwise pose, bit for bit (pose_out may be NULL with evaluate_only)
 *      Status is an output only: a failed step passes its pose through, so a loop over steps needs no state.  Non-positive sizes,
 *      B > 65535, H * W >= 2^31, without frame an Ft that is neither 1 nor B, a tau that is not finite and positive, a damping
 *      that is not finite and >= 0, null pointers, a workspace that is not 16-byte aligned and pose_out == pose are refused (-1,
 *      tp_last_error) before anything is launched.  No input value (NaN, Inf, a frame index out of range, huge poses) causes an
 *      access out of bounds: frame is the only index read from memory, and it is clamped.  Two launches.  No allocation, no host
 *      synchronisation; outputs and workspace must not overlap inputs.  Safe to capture.
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_photo_align_args {
  const float* zbuf;         /* [B,H,W] K19's depth of the mesh at pose: mm, <= 0 or NaN: background */
  const float* rgb;          /* [B,H,W,3] K19's colours of the vertex-coloured mesh at pose */
  const float* pose;         /* [B,3,4] the pose zbuf and rgb were rendered at */
  const float* intr;         /* [B,3,3] */
  const float* image;        /* [Ft,H,W,3] the photograph, channels last, in rgb's units */
  const int32_t* frame;      /* [B] index into image (and mask), or NULL: b when Ft == B, 0 when Ft == 1 */
  const uint8_t* mask;       /* [Ft,H,W] or NULL; 0: the pixel is skipped */
  int B, Ft, H, W;
  float tau;                 /* finite, > 0: the largest colour distance |o - c| of a kept pixel */
  float damping;             /* finite, >= 0: relative Levenberg damping of the diagonal */
  int evaluate_only;         /* non-zero: inliers, rms and status of pose; no step */
  float* pose_out;           /* [B,3,4] out; may be NULL with evaluate_only; must not be pose */
  int32_t* inliers;          /* [B] out */
  float* rms;                /* [B] out, colour units */
  int32_t* status;           /* [B] out: 0 ok, 1 fewer than 6 kept pixels, 3 not positive definite */
  void* workspace;           /* tp_photo_align_workspace_bytes(B, H, W) bytes, 16-byte aligned; needs no clearing */
} tp_photo_align_args;
size_t tp_photo_align_workspace_bytes(int B, int H, int W);  /* 256 * B * ceil(H * W / 1024), rounded up to 16; 0 for non-positive sizes */
int tp_photo_align_step(const tp_photo_align_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K31a the exact signed Euclidean distance field of F masks (texpose_amd/silhouette.py; restated in tests/silhouette_ref.py; the
 *      project's own kernel, no reference code).  mask [F,H,W] uint8, any non-zero value is "set"; sdf [F,H,W]
 *      float32.  For pixel p of a plane, d2_set(p) = min |p - q|^2 over the set pixels q of that plane and d2_clear(p) the same over
 *      its clear pixels, both integers; where a plane has no such pixel the value is the sentinel H^2 + W^2, larger than any real
 *      squared distance.  Pixels outside the image do not exist: they are neither set nor clear.
 *        sdf = mask == 0 ? sqrtf((float)d2_set) - 0.5f : -(sqrtf((float)d2_clear) - 0.5f)
 *      (sqrtf correctly rounded): positive outside the mask, negative inside, the zero level half-way between a set pixel and its
 *      clear neighbour; always finite.  Integer minima do not depend on the order they are taken in: the field is a function of the
 *      mask alone.  Two launches: a sweep down and up every column (the vertical distances to the nearest set and the nearest clear
 *      pixel, 16 bits each, into the workspace), then one workgroup per row, which holds the row's pairs in LDS and takes
 *      min over j' of (j - j')^2 + g[j']^2 for each of its pixels, outwards from j until (j - j')^2 reaches the best so far.
 *      Non-positive sizes, H or W > 8192, F * H * W >= 2^31, null pointers, a workspace that is not 16-byte aligned and an sdf that
 *      overlaps mask are refused (-1, tp_last_error) before anything is launched.  No atomics, no allocation, no host
 *      synchronisation.  Safe to capture.
 * ------------------------------------------------------------------------------------------ */
size_t tp_mask_sdf_workspace_bytes(int F, int H, int W);   /* 4 * F * H * W, rounded up to 16; 0 for non-positive sizes; needs no clearing */
int tp_mask_sdf(const uint8_t* mask, float* sdf, int F, int H, int W, void* workspace, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K31c the field of a mask with UNKNOWN pixels (texpose_amd/silhouette.py; restated in tests/occlusion_ref.py; the project's own
 *      kernel, no reference code).  known [F,H,W] uint8, non-zero: the pixel's mask value is a measurement.  Per
 *      plane a pixel is SET (mask != 0 and known != 0), CLEAR (mask == 0 and known != 0) or UNKNOWN (known == 0, whatever mask
 *      holds: behind an occluder, say).  d2_set(p) and d2_clear(p) are K31a's integers taken over the SET and the CLEAR pixels only,
 *      the sentinel H^2 + W^2 where the plane has none; an unknown pixel is neither, so no distance is ever measured to it.
 *        sdf = SET ? -(sqrtf((float)d2_clear) - 0.5f) : CLEAR ? sqrtf((float)d2_set) - 0.5f : quiet NaN
 *      (sqrtf correctly rounded).  K31b drops a rim pixel whose field value or any of whose four neighbours' values is not finite and
 *      counts a non-finite value as outside: it takes this field as it is.  With known all non-zero the result is tp_mask_sdf's bit
 *      for bit.  The workspace is tp_mask_sdf_workspace_bytes'; the refusals are K31a's with known among the pointers, and an sdf that
 *      overlaps known.  The same two launches (an unknown pixel advances both distances of the column sweep, and the row kernel
 *      knows it by neither being 0), no atomics, integer minima: a function of (mask, known) alone.  Safe to capture.
 * ------------------------------------------------------------------------------------------ */
int tp_mask_sdf_known(const uint8_t* mask, const uint8_t* known, float* sdf, int F, int H, int W, void* workspace, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K32  who hides whom, from the instance masks of ONE frame (texpose_amd/silhouette.py; restated in tests/occlusion_ref.py; the
 *      project's own kernel, no reference code).  sdf [N,H,W] holds tp_mask_sdf's fields of the frame's N instance
 *      masks, known [N,H,W] uint8 is written.  near(m,p) = sdf[m,p] <= band_px - 0.5f, in fp32 as written (a NaN is not near): pixel
 *      p lies within band_px pixels of a set pixel of instance m; band_px = 0 is the instance's own pixels.
 *        known[n,p] = 0 iff near(m,p) for some m != n;  else 1
 *      Conservative by construction: along the contour between two touching instances both lose the pixels within band_px of the
 *      other, the one in front too, whose contour there is real.  One launch: a thread owns four consecutive flat pixels, walks the
 *      N planes once counting the near instances and keeping the index of one, then writes the N bytes: 0 iff count > 1 or (count
 *      == 1 and index != n).  Non-positive sizes, N > 65535, N * H * W >= 2^31, null pointers, a band_px that is not finite and
 *      >= 0 and a known that overlaps sdf are refused (-1, tp_last_error) before the launch.  No workspace, no atomics.  Safe to
 *      capture.
 * ------------------------------------------------------------------------------------------ */
int tp_mask_known_from_others(const float* sdf, uint8_t* known, int N, int H, int W, float band_px, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K31b one step of batched silhouette alignment: B poses refined against the outline of a mask (texpose_amd/silhouette.py; restated
 *      in tests/silhouette_ref.py; the project's own step, no reference code).  zbuf is K19's depth of the mesh
 *      rendered at pose, sdf the signed distance field of the measured mask (tp_mask_sdf's, or any field in pixels that is negative
 *      inside); the call takes one damped Gauss-Newton step of the update x' = x + w x x + v in the camera frame (parameters
 *      (w, v), as tp_photo_align_step): a surface point on the rendered rim moves in the image, and the field says how far from the
 *      measured outline it would land.  A pixel is COVERED iff its z = zbuf[b,i,j] is > 0 and finite.  Per pixel (row i, column j)
 *      of image b, with K = intr[b] (fx = K_00, fy = K_11, cx = K_02, cy = K_12) and the plane fr = frame ? frame[b] CLAMPED into
 *      [0, Ft) : (Ft == 1 ? 0 : b), everything in fp64 from the fp32 inputs, evaluated as written (no contraction):
 *        1. skipped unless 1 <= i <= H - 2 and 1 <= j <= W - 2 (an image with H < 3 or W < 3 keeps nothing) and the pixel is covered
 *        2. skipped unless it is a RIM pixel: at least one of its four neighbours (i,j-1), (i,j+1), (i-1,j), (i+1,j) is not covered
 *           (a NaN neighbour is not covered)
 *        3. skipped where mask is given and mask[fr,i,j] == 0
 *        4. d = sdf[fr,i,j] and the four neighbours sdf[fr,i,j-1], sdf[fr,i,j+1], sdf[fr,i-1,j], sdf[fr,i+1,j];  skipped unless all
 *           five are finite
 *        5. r = d + 0.5 (a rendered rim pixel that sits on the mask's own rim reads 0);  kept iff |r| <= tau_px
 *        6. gx = 0.5 (sdf[fr,i,j+1] - sdf[fr,i,j-1]),  gy = 0.5 (sdf[fr,i+1,j] - sdf[fr,i-1,j]),
 *           rx = ((j + 0.5) - cx) / fx,  ry = ((i + 0.5) - cy) / fy,  P = (z rx, z ry, z),
 *           a = (gx fx / z,  gy fy / z,  -((gx fx) rx + (gy fy) ry) / z),  J = [P x a, a]
 *      and the 29 sums of tp_pnp_refine over the rows (J, r) of the kept pixels: the 21 upper-triangle entries of J^T J (row-major),
 *      the 6 of J^T r, sum r^2 and the count.  A thread owns four consecutive flat pixels (ascending), a workgroup 1024; butterfly
 *      sums inside a wave, the four waves in ascending order, one record per workgroup, the records in ascending order: no atomics,
 *      the outputs are a function of the inputs alone, bit-identical from run to run and under graph replay.  Per image:
 *        inliers = count, the kept rim pixels;  rms = sqrt(sum r^2 / count) in pixels (NaN at count 0): both describe `pose`
 *        status  = 1 where count < 6; else 3 where J^T J is NOT POSITIVE DEFINITE by tp_pnp_refine's pivot rule (a Cholesky pivot
 *                  that is not finite or <= 1e-10 x its diagonal entry), or, without evaluate_only, where the damped matrix does
 *                  not factor or the stepped pose is not finite in fp32; else 0
 *        pose_out = (status == 0 and not evaluate_only): (J^T J + damping diag(J^T J)) delta = -J^T r solved by Cholesky,
 *                  R <- exp(w) R, t <- exp(w) t + v with Rodrigues' formula, Gram-Schmidt on R's first two columns (the third
 *                  their cross product), rounded to fp32;  otherwise pose, bit for bit (pose_out may be NULL with evaluate_only)
 *        inter   = the pixels (all H * W, the border included) that are covered AND have sdf[fr,i,j] < 0;  uni = those where either
 *                  holds.  A sdf value that is not finite counts as outside; mask is ignored.  Exact integer counts (ballots and
 *                  popcounts, added as integers), the same from run to run.  They describe `pose`: its IoU with the measured mask
 *                  is inter / uni.
 *      Status is an output only: a failed step passes its pose through, so a loop over steps needs no state.  Non-positive sizes,
 *      B > 65535, H * W >= 2^31, without frame an Ft that is neither 1 nor B, a tau_px that is not finite and positive, a damping
 *      that is not finite and >= 0, null pointers, a workspace that is not 16-byte aligned and pose_out == pose are refused (-1,
 *      tp_last_error) before anything is launched.  No input value (NaN, Inf, a frame index out of range, huge poses) causes an
 *      access out of bounds: frame is the only index read from memory, and it is clamped; the interior test keeps every neighbour
 *      read inside the plane.  Three launches.  No allocation, no host synchronisation; outputs and workspace must not overlap
 *      inputs.  Safe to capture.
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_silhouette_align_args {
  const float* zbuf;         /* [B,H,W] K19's depth of the mesh at pose: mm, <= 0 or NaN: background */
  const float* pose;         /* [B,3,4] the pose zbuf was rendered at */
  const float* intr;         /* [B,3,3] */
  const float* sdf;          /* [Ft,H,W] signed distance to the measured outline in pixels, negative inside (tp_mask_sdf) */
  const int32_t* frame;      /* [B] index into sdf (and mask), or NULL: b when Ft == B, 0 when Ft == 1 */
  const uint8_t* mask;       /* [Ft,H,W] or NULL; 0: the pixel gives no row */
  int B, Ft, H, W;
  float tau_px;              /* finite, > 0: the largest distance |d + 0.5| between a kept rim pixel and the measured outline */
  float damping;             /* finite, >= 0: relative Levenberg damping of the diagonal */
  int evaluate_only;         /* non-zero: inliers, rms, status, inter and uni of pose; no step */
  float* pose_out;           /* [B,3,4] out; may be NULL with evaluate_only; must not be pose */
  int32_t* inliers;          /* [B] out */
  float* rms;                /* [B] out, pixels */
  int32_t* status;           /* [B] out: 0 ok, 1 fewer than 6 kept pixels, 3 not positive definite */
  int32_t* inter;            /* [B] out: covered pixels inside the measured mask */
  int32_t* uni;              /* [B] out: pixels covered or inside the measured mask */
  void* workspace;           /* tp_silhouette_align_workspace_bytes(B, H, W) bytes, 16-byte aligned; needs no clearing */
} tp_silhouette_align_args;
size_t tp_silhouette_align_workspace_bytes(int B, int H, int W);  /* 256 * B * ceil(H * W / 1024), rounded up to 16; 0 for non-positive sizes */
int tp_silhouette_align_step(const tp_silhouette_align_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K33  one JOINT step of the render-and-compare refiners: the residual rows of K31b (silhouette), K30 (photometric) and K29 (depth)
 *      in ONE normal system (texpose_amd/joint.py; restated in tests/joint_ref.py; the project's own step, no reference code; DESIGN
 *      section 23).  The three terms share the six parameters (w, v), the 29 fp64 sums and the record per (image, 1024-pixel tile);
 *      each term that is present (its pointer is not NULL) is its own args struct, unchanged, with its own planes, threshold, frame
 *      map, mask, outputs and workspace.  The call
 *        1. evaluates every present term exactly as that term's own step would with evaluate_only = 1: the term's inliers, rms and
 *           status (and inter / uni of the silhouette) and the records in its workspace are bit for bit those of the standalone
 *           call.  The term's pose_out and evaluate_only fields are ignored (nothing is written through that pose_out);
 *        2. per image gathers each term's records in ascending tile order into that term's sums S_t[0 .. 28], terms in the order
 *           silhouette, photometric, depth, and forms over the terms that are present AND have a weight > 0
 *             sum[k] = w_a S_a[k] (+ w_b S_b[k] (+ w_c S_c[k]))     for k = 0 .. 27, in fp64 as written (no contraction)
 *           with the float weights widened to fp64.  A term that is absent or has weight 0 is skipped, not added as zero.
 *           inliers = the sum of the counts S_t[28] of those terms;  chi2 = sum[27], rounded to fp32: the weighted sum of squares;
 *        3. applies K29's rules to the combined sums: status 1 where inliers < 6; else 3 where the combined J^T J is not positive
 *           definite by the pivot rule, or, without evaluate_only, where the damped matrix does not factor or the stepped pose is not
 *           finite in fp32; else 0.  pose_out = (status == 0 and not evaluate_only) the damped step of K29 on the combined sums,
 *           rounded to fp32; otherwise pose, bit for bit (pose_out may be NULL with evaluate_only).
 *      A weight is 1 / sigma^2 of that term's residual unit (pixels, colour units, mm).  With one term present at weight exactly 1
 *      pose_out and status are that term's own step's, bit for bit.  Refused (-1, tp_last_error) before anything is launched: a
 *      null args; no term present, or none with a weight > 0; a weight that is negative or not finite; a damping that is not finite
 *      and >= 0; null pose, status, inliers or chi2; pose_out missing without evaluate_only, or overlapping pose; a present term
 *      whose B or pose differs from args', or whose H, W or intr differs from another term's; two terms whose workspaces overlap;
 *      and whatever the term's own step refuses.  Per present term that term's reduce launches and its evaluating solve, then one
 *      launch of the joint solve (grid B, one wave).  No atomics, no allocation, no host synchronisation; bit-identical from run to
 *      run.  Safe to capture.
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_joint_align_args {
  int B;
  const float* pose;         /* [B,3,4] the pose every term's planes were rendered at (each term's pose must be this pointer) */
  float w_sil, w_photo, w_icp; /* finite, >= 0: 1 / sigma^2 of the term's residual unit; 0: evaluated, not in the step */
  float damping;             /* finite, >= 0: relative Levenberg damping of the combined diagonal */
  int evaluate_only;         /* non-zero: inliers, chi2 and status of pose; no step */
  float* pose_out;           /* [B,3,4] out; may be NULL with evaluate_only; must not overlap pose */
  int32_t* status;           /* [B] out: 0 ok, 1 fewer than 6 kept pixels over the weighted terms, 3 not positive definite */
  int32_t* inliers;          /* [B] out: the kept pixels of the weighted terms, added */
  float* chi2;               /* [B] out: the weighted sum of squared residuals */
} tp_joint_align_args;
int tp_joint_align_step(const tp_joint_align_args* j,
                        const tp_silhouette_align_args* sil,   /* may be NULL */
                        const tp_photo_align_args* photo,      /* may be NULL */
                        const tp_depth_icp_args* icp,          /* may be NULL */
                        tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K35  shade the pixels of K19's face plane from a per-face texel texture ("mesh colours": texpose_amd/face_texels.py; restated in
 *      tests/face_texels_ref.py; the project's own step, no reference code).  Resolution R, 1 <= R <=
 *      TP_FACE_TEXEL_MAX_R.  Face f with vertices (v0, v1, v2) in its own order carries the nodes (i, j), i, j >= 0, i + j <= R; node
 *      (i, j) sits at the barycentric weights ((R - i - j) / R, i / R, j / R) and is stored at n(i, j) = j (R + 1) - j (j - 1) / 2 + i
 *      of the face's T(R) = (R + 1)(R + 2) / 2 texels: texels is [F, T, 3].  Per pixel (row i, column j) of image b with f = face:
 *        u_k, v_k, 1 / z_k of the face's vertices in fp64 from verts, faces, pose[b], intr[b] exactly as K19's face setup forms them
 *        area   = (u_1 - u_0)(v_2 - v_0) - (v_1 - v_0)(u_2 - u_0)                                   (twice the signed area)
 *        b_k    = ((u_e - u_s)(py - v_s) - (v_e - v_s)(px - u_s)) / area,  s = (k + 1) % 3, e = (k + 2) % 3, (px, py) = (j + 0.5, i + 0.5)
 *        t_k    = b_k * (1 / z_k),  w_k = t_k / ((t_0 + t_1) + t_2);  w_k < 0 becomes 0;  w_k = w_k / ((w_0 + w_1) + w_2)
 *        a = R w_1, b = R w_2, ci = min(floor(a), R - 1), cj = min(floor(b), R - 1 - ci), fa = a - ci, fb = b - cj
 *        fa + fb > 1 and ci + cj <= R - 2:  c = ((fa + fb) - 1) N(ci+1, cj+1) + (1 - fb) N(ci+1, cj) + (1 - fa) N(ci, cj+1)
 *        otherwise:                         c = ((1 - fa) - fb) N(ci, cj) + fa N(ci+1, cj) + fb N(ci, cj+1)
 *      (a cell of the last diagonal, ci + cj = R - 1, has no upper triangle: there fa + fb exceeds 1 by rounding alone), the three
 *      products added left to right.  Piecewise linear and continuous; at R = 1 the perspective-correct vertex interpolation.  Every
 *      step is fp64, evaluated as written (no contraction), and rounded to fp32 once.  rgb = (0, 0, 0), and nothing else is read,
 *      for face < 0 or >= F, a vertex index outside 0 .. V-1, a vertex with z <= 0 or a non-finite camera-frame coordinate, |area| <=
 *      1e-10 or not finite, and any non-finite w_k or colour.  Nothing is read out of bounds for any face plane or pose.  Point
 *      sampling (the minification filter is K43's tp_face_texel_shade_mip, below, not this entry point).  One launch, one thread
 *      per pixel; no LDS, no atomics, no workspace, no allocation, no host
 *      synchronisation; the output is a function of the inputs alone.  Non-positive sizes, R outside 1 .. TP_FACE_TEXEL_MAX_R,
 *      H * W >= 2^31, F * T >= 2^31, B * ceil(H W / 256) >= 2^31 and null pointers are refused (-1, tp_last_error) and launch
 *      nothing.  Safe to capture.
 * ------------------------------------------------------------------------------------------ */
#define TP_FACE_TEXEL_MAX_R 64
typedef struct tp_face_texel_shade_args {
  const float* verts;        /* [V,3] model frame, mm */
  const int32_t* faces;      /* [F,3] */
  const float* texels;       /* [F,T,3], T = tp_face_texel_count(R) */
  const float* pose;         /* [B,3,4] [R|t] model -> camera (K19's convention) */
  const float* intr;         /* [B,3,3] */
  const int32_t* face;       /* [B,H,W] K19's face plane (any values: out-of-range entries shade to zero) */
  int B, H, W, V, F, R;
  float* rgb;                /* [B,H,W,3] out */
} tp_face_texel_shade_args;
int tp_face_texel_count(int R);                           /* T(R); 0 for R outside 1 .. TP_FACE_TEXEL_MAX_R */
int tp_face_texel_shade(const tp_face_texel_shade_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K36  the adjoint of K35 with respect to the texels (texpose_amd/face_texels.py: shade_nodes, FaceTexelFitter; restated in
 *      tests/face_texel_fit_ref.py; the project's own step).  K35 is linear in the texels: a pixel p of face f that
 *      K35 shades by rule reads the three slots and weights of its cell,
 *        fa + fb > 1 and ci + cj <= R - 2:  (n(ci+1, cj+1), (fa + fb) - 1), (n(ci+1, cj), 1 - fb), (n(ci, cj+1), 1 - fa)
 *        otherwise:                         (n(ci, cj), (1 - fa) - fb),     (n(ci+1, cj), fa),     (n(ci, cj+1), fb)
 *      and the adjoint adds w_k grad_rgb[p] (3 channels) to the destination d(f, n_k): the slot f T + n_k itself (N = F T destinations)
 *      when node_index is NULL, node_index[f T + n_k] otherwise (N = U destinations; an entry outside 0 .. U-1 is skipped).  weight,
 *      where given, is the same sum with grad_rgb = 1: the coverage of each destination (the lumped diagonal of S^T S).  A pixel
 *      contributes nothing where K35 writes zeros by its geometric rules (face < 0 or >= F, a vertex index outside 0 .. V-1, a vertex
 *      with z <= 0 or a non-finite camera-frame coordinate, |area| <= 1e-10 or not finite, a non-finite w_k) and nothing where a
 *      component of its grad_rgb is not finite.  K35's "non-finite colour -> zero" rule depends on the texel values: the adjoint
 *      reads no texels and ignores it.
 *      Deterministic without float atomics -- 64-bit fixed point; integer addition is associative, so neither the arrival order
 *      nor a graph replay changes a bit.  With gmax = the maximum of |grad_rgb| over the components of the contributing pixels (found
 *      on the device: an unsigned atomic maximum of the floats' bit patterns) and e = max(floor(log2 gmax), -126), every contribution
 *      is q = llrint((w_k (double)g_c) 2^(36 - e)): an fp64 product rounded to nearest even, |q| <= 2^37 (1 + 2^-50), added to an
 *      int64 by an integer atomic; the weights use llrint(w_k 2^36).  At the end grad = (float)((double)sum 2^(e - 36)), rounded
 *      once; weight likewise; gmax = 0 gives grad = 0.  The weights of one pixel are >= -2^-50 and add up to 1 within 2^-50, so a
 *      pixel adds at most 2^37 (1 + 2^-49) in magnitude to any one destination whatever node_index holds, and B H W <= 2^25 pixels
 *      stay below 2^63: no sum can overflow.  Each q is within 1/2 of its exact value, so a result is within n_d gmax 2^-37 (the
 *      coverage: n_d 2^-37) of the exact sum over the n_d contributions to d, plus its one rounding to fp32.
 *      Four launches on the stream (one memset of the workspace, maximum, scatter, finalise), one thread per pixel; no host
 *      synchronisation, no allocation; safe to capture.  Everything K35 refuses, B H W > 2^25, U <= 0 with a node index, 3 N >= 2^31,
 *      a null or not 8-byte aligned workspace and a null grad_rgb or grad are refused (-1, tp_last_error) and launch nothing.
 *      Left out: gradients with respect to the pose or the vertices, second order, one R per face, the adjoint of K43's
 *      minification filter (the forward has one since K43, below).
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_face_texel_shade_bwd_args {
  const float* verts;        /* [V,3] as K35 */
  const int32_t* faces;      /* [F,3] */
  const float* pose;         /* [B,3,4] */
  const float* intr;         /* [B,3,3] */
  const int32_t* face;       /* [B,H,W] K19's face plane (any values) */
  const float* grad_rgb;     /* [B,H,W,3] */
  const int32_t* node_index; /* [F,T] or NULL */
  int B, H, W, V, F, R, U;   /* U: destinations when node_index is given; ignored otherwise (N = F * T) */
  void* workspace;           /* tp_face_texel_shade_bwd_workspace(N, weight != NULL) bytes, 8-byte aligned; cleared by the call */
  float* grad;               /* [N,3] out */
  float* weight;             /* [N] out or NULL */
} tp_face_texel_shade_bwd_args;
size_t tp_face_texel_shade_bwd_workspace(int64_t N, int want_weight);      /* 8 (3 N + (want_weight ? N : 0) + 1); 0 for N <= 0 or 3 N >= 2^31 */
int tp_face_texel_shade_bwd(const tp_face_texel_shade_bwd_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K37  per-image, per-channel gain and bias between a rendering and its photograph (texpose_amd/ops/refine.py: photo_exposure;
 *      restated in tests/photo_exposure_ref.py; the project's own step, no reference code).  zbuf / rgb are K19's
 *      planes at the current poses; the call fits  o_k ~ g_k c_k + b_k  per image b and channel k by least squares over the pixels
 *      the fit that came in (gain_in, bias_in; NULL: gain 1, bias 0) explains within tau, and, where rgb_out is given, applies the
 *      new fit to the rendering, so that K30 / K33 compare colours under the photograph's exposure.  No neighbour pixel, pose or
 *      intrinsics are read.  Per pixel (row i, column j) of image b, with the photograph fr = frame ? frame[b] CLAMPED into [0, Ft)
 *      : (Ft == 1 ? 0 : b), everything in fp64 from the fp32 inputs, evaluated as written (no contraction):
 *        1. skipped unless 1 <= i <= H - 2 and 1 <= j <= W - 2                       (K30's interior)
 *        2. z = zbuf[b,i,j];           skipped unless z > 0 and finite
 *        3. skipped where mask is given and mask[fr,i,j] == 0
 *        4. c_k = rgb[b,i,j,k], o_k = image[fr,i,j,k] for k = 0, 1, 2;  skipped unless all six values are finite
 *        5. r_k = o_k - (a_k c_k + d_k) with (a, d) = (gain_in[b], bias_in[b]);  kept iff (r_0^2 + r_1^2) + r_2^2 <= tau * tau
 *      Sixteen sums over the kept pixels: [0] n (+ 1 per pixel) and, for channel k, [1 + 5 k ..]: c_k, o_k, c_k c_k, c_k o_k,
 *      o_k o_k.  A thread owns four consecutive flat pixels (ascending, channels ascending), a workgroup 1024; butterfly sums
 *      inside a wave, the four waves in ascending order, one 32-double record per workgroup (entries 16 .. 31 are zero), the
 *      records in ascending order: K30's order; no atomics, the outputs are a function of the inputs alone, bit-identical from run
 *      to run and under graph replay.  Per image and channel, in fp64 as written (Sc, So, Scc, Sco, Soo the channel's sums):
 *        mc = Sc / n;  mo = So / n;  var = Scc / n - mc mc;  cov = Sco / n - mc mo;  voo = Soo / n - mo mo
 *        var > min_var:  g = min(max(cov / var, gain_min), gain_max);  bit k of flags where g != cov / var      (the clamp acted)
 *        otherwise:      g = 1;                                         bit 3 + k of flags                       (a flat channel)
 *        b = mo - g mc;   sse_k = n ((voo - 2 (g cov)) + (g g) var)                  (the squared error at (g, b), from the sums)
 *      count = n;  rms = sqrt(max(0, (sse_0 + sse_1) + sse_2) / n) in colour units, of the fit just made (NaN at n = 0);
 *        status = 1 where n < 6; else 3 where one of g_k, b_k or rms rounded to fp32 is not finite; else 0
 *        gain, bias = (g, b) rounded to fp32 where status == 0;  otherwise gain_in, bias_in bit for bit (1 and 0 where NULL);
 *        flags are those of the fit just made whatever the status
 *      Apply, where rgb_out is given: a pixel with zbuf > 0 and finite (border pixels included) becomes
 *        rgb_out[b,i,j,k] = gain[b,k] * rgb[b,i,j,k] + bias[b,k]   as two fp32 operations (a product, then a sum)
 *      with the gain and bias the call just wrote; every other pixel is copied bit for bit, and with rgb_out == rgb is not written.
 *      Status is an output only: a failed fit passes the fit that came in through, so a loop needs no state.  Three launches on
 *      the stream (reduce, solve, apply; two without rgb_out).  Non-positive sizes, B > 65535, H * W >= 2^31, without frame an Ft
 *      that is neither 1 nor B, a tau that is not finite and positive, gain_min / gain_max outside 0 < gain_min <= 1 <= gain_max <
 *      inf, a min_var that is not finite and >= 0, null pointers, a workspace that is not 16-byte aligned, an rgb_out that overlaps
 *      rgb without being rgb, and gain or bias overlapping gain_in or bias_in are refused (-1, tp_last_error) before anything is
 *      launched.  No input value causes an access out of bounds: frame is the only index read from memory, and it is clamped.  No
 *      allocation, no host synchronisation; outputs and workspace must not overlap inputs otherwise.  Safe to capture.
 *      Left out: a gain shared by the channels, a spatially varying model, exact elimination inside the pose step's system.
 * ------------------------------------------------------------------------------------------ */
#define TP_EXPOSURE_CLAMPED 1  /* flags: << k, channel k's gain was clamped into [gain_min, gain_max] */
#define TP_EXPOSURE_FLAT 8     /* flags: << k, channel k's variance was <= min_var: gain 1 */
typedef struct tp_photo_exposure_args {
  const float* zbuf;         /* [B,H,W] K19's depth at the current poses: <= 0 or NaN: background */
  const float* rgb;          /* [B,H,W,3] K19's colours at the current poses */
  const float* image;        /* [Ft,H,W,3] the photograph, channels last */
  const int32_t* frame;      /* [B] index into image (and mask), or NULL: b when Ft == B, 0 when Ft == 1 */
  const uint8_t* mask;       /* [Ft,H,W] or NULL; 0: the pixel is skipped */
  const float* gain_in;      /* [B,3] or NULL (1): the fit the keep rule judges by */
  const float* bias_in;      /* [B,3] or NULL (0) */
  int B, Ft, H, W;
  float tau;                 /* finite, > 0: the largest colour distance |o - (a c + d)| of a kept pixel */
  float gain_min, gain_max;  /* 0 < gain_min <= 1 <= gain_max, finite */
  float min_var;             /* finite, >= 0, colour units squared: a channel whose variance is not above it keeps gain 1 */
  float* gain;               /* [B,3] out */
  float* bias;               /* [B,3] out */
  int32_t* count;            /* [B] out */
  float* rms;                /* [B] out, colour units */
  int32_t* status;           /* [B] out: 0 ok, 1 fewer than 6 kept pixels, 3 not finite */
  int32_t* flags;            /* [B] out: TP_EXPOSURE_CLAMPED << k | TP_EXPOSURE_FLAT << k */
  float* rgb_out;            /* [B,H,W,3] out, rgb itself (in place) or NULL (fit only) */
  void* workspace;           /* tp_photo_exposure_workspace_bytes(B, H, W) bytes, 16-byte aligned; needs no clearing */
} tp_photo_exposure_args;
size_t tp_photo_exposure_workspace_bytes(int B, int H, int W);  /* 256 * B * ceil(H * W / 1024), rounded up to 16; 0 for non-positive sizes */
int tp_photo_exposure(const tp_photo_exposure_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K38  one level down an image pyramid, for the photograph, the rendering and the mask of the photometric alignment
 *      (texpose_amd/ops/refine.py: image_down, surface_down, mask_down; restated in tests/photo_pyramid_ref.py; the project's own step,
 *      no reference code).  A plane of H x W becomes one of h x w = (H / 2) x (W / 2), rounded down: an odd last
 *      row or column is only ever a tap.  Coarse pixel (I, J) has its centre at fine coordinate 2 (J + 1/2, I + 1/2), so level l's
 *      intrinsics are K with rows 0 and 1 times 2^-l, and K30's + .5 pixel-centre convention holds at every level.
 *      The filter is separable and even: the taps of coarse row I are the fine rows clamp(2 I - 1 + a, 0, H - 1), a = 0 .. 3, those
 *      of coarse column J the fine columns clamp(2 J - 1 + b, 0, W - 1), b = 0 .. 3, with the weights w = (1, 3, 3, 1) / 8.  In fp64
 *      from the fp32 inputs, evaluated as written (no contraction), x_ab the tap of row a and column b:
 *        s_a = ((w_0 x_a0 + w_1 x_a1) + w_2 x_a2) + w_3 x_a3        for a = 0 .. 3
 *        y   = ((w_0 s_0 + w_1 s_1) + w_2 s_2) + w_3 s_3            rounded to fp32 once
 *      per channel.  The outputs are a function of the inputs alone: bit-identical from run to run and under graph replay.
 *      tp_image_down:   image [N,H,W,3] -> [N,h,w,3], y of every channel; non-finite taps propagate as IEEE arithmetic gives
 *                       (K30 drops such pixels).
 *      tp_surface_down: zbuf [N,H,W], rgb [N,H,W,3] (K19's planes) -> [N,h,w], [N,h,w,3].  A tap is a surface iff z > 0 and finite
 *                       (K30's test); a coarse pixel is a surface iff ALL 16 taps are.  There zbuf_out = y of z and rgb_out = y of
 *                       each channel; everywhere else zbuf_out = -1 and rgb_out = 0 (K19's background), and rgb is not read.  The rim
 *                       is eroded by the filter's footprint: exactly the coarse pixels whose photographed value mixes in background.
 *                       With the photograph equal to the rendering composited over any background, a surface pixel of every level
 *                       holds the same value on both sides bit for bit: the same 16 values through the same arithmetic.
 *      tp_mask_down:    mask [N,H,W] uint8 -> [N,h,w]: 1 iff all 16 taps are non-zero, else 0.
 *      One launch each on the stream; no atomics, no allocation, no workspace, no host synchronisation; safe to capture.  No index is
 *      read from memory and every tap is clamped.  N outside 1 .. 65535, H < 2, W < 2, H * W >= 2^31, null pointers and an output
 *      overlapping an input (or the other output) are refused (-1, tp_last_error) before anything is launched.
 *      Left out: other filters or factors than 2, a rasteriser at the reduced size (the rasteriser point-samples
 *      the texture while the photograph is filtered, and the loop loses images it otherwise solves).
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_pyramid_down_args {
  const float* zbuf;     /* [N,H,W] tp_surface_down: K19's depth, <= 0 / NaN / Inf: no surface; NULL for the other two */
  const float* rgb;      /* [N,H,W,3] tp_surface_down: K19's colours; tp_image_down: the photograph, channels last; NULL for tp_mask_down */
  const uint8_t* mask;   /* [N,H,W] tp_mask_down; NULL for the other two */
  int N, H, W;
  float* zbuf_out;       /* [N,H/2,W/2] out, tp_surface_down */
  float* rgb_out;        /* [N,H/2,W/2,3] out, tp_surface_down and tp_image_down */
  uint8_t* mask_out;     /* [N,H/2,W/2] out, tp_mask_down */
} tp_pyramid_down_args;
int tp_image_down(const tp_pyramid_down_args* args, tp_stream_t stream);    /* reads rgb, writes rgb_out */
int tp_surface_down(const tp_pyramid_down_args* args, tp_stream_t stream);  /* reads zbuf and rgb, writes zbuf_out and rgb_out */
int tp_mask_down(const tp_pyramid_down_args* args, tp_stream_t stream);     /* reads mask, writes mask_out */

/* ------------------------------------------------------------------------------------------
 * K39  MULTI-VIEW pose refinement: ONE object pose per group of views whose cameras are known (texpose_amd/multiview.py; restated in
 *      tests/multiview_ref.py; the project's own step, no reference code).
 *      Views i = 0 .. B-1; cam [B,3,4] C_i = [Rc|tc], world -> camera i, fixed; group [B] int32 in 0 .. Gr-1; model [Gr,3,4] M_g,
 *      model -> world, the unknowns.  View i is rendered and evaluated at T_i = C_i o M_group[i].
 *      COMPOSE (tp_pose_compose, a thread per view): T_i = [Rc Rm | Rc tm + tc] in fp64 from the fp32 inputs,
 *        T[r][c] = (Rc[r][0] M[0][c] + Rc[r][1] M[1][c]) + Rc[r][2] M[2][c]      for c = 0 .. 3, and for c = 3 then + tc[r],
 *      every dot product left to right as written (no contraction), rounded to fp32 once.  If cam[i] is bit-exactly [I|0] (the words
 *      of 1.0f on the diagonal, of +0.0f elsewhere) T_i is model[group[i]] bit for bit: a copy, since the arithmetic would turn a -0.0
 *      into +0.0.  A group id out of range is clamped into 0 .. Gr-1; nothing is read past an array.
 *      CHANGE OF VARIABLES: K29's step moves a view by x' = exp(w) x + v in the CAMERA frame; perturb M the same way in the WORLD frame
 *      by d = (w, v).  To first order view i moves by xi_i = A_i d with the 6x6
 *        A_i = [[Rc, 0], [[tc]x Rc, Rc]]          ([tc]x the cross-product matrix; [tc]x Rc formed with dots as above)
 *      so with S_i the view's combined sums, H_i its 6x6 matrix and g_i its six J^T r the view contributes
 *        H'_i = A_i^T H_i A_i,   g'_i = A_i^T g_i,   chi2 and the count unchanged.
 *      In fp64, A from the fp32 cam: P = H A, then Q = A^T P, each entry a sum over the inner index ascending starting from its first
 *      product; the upper triangle of Q is taken; g' = A^T g likewise.  A view whose cam is bit-exactly [I|0] is not transformed: its
 *      sums pass through bit for bit.
 *      A VIEW'S COMBINED SUMS are K33's, unchanged: every present term is evaluated with evaluate_only = 1 at `pose` (= T, the caller
 *      composes it), its records gathered in ascending tile order, terms in the order silhouette, photometric, depth, and
 *      w_a S_a (+ w_b S_b (+ w_c S_c)) formed over the present terms with weight > 0; the count is not weighted.
 *      A GROUP'S SYSTEM: the member views of group g are member[group_start[g] .. group_start[g+1] - 1] (view indices, ascending inside
 *      a group); their transformed records are added in that order, the first one assigned; K29's rules (count, pivot rule, damped
 *      step, fp32 rounding) run unchanged on the sum with the current pose model[g]: fewer than six rows in the whole group: status 1;
 *      the pivot rule decides between 0 and 3; otherwise the step.  A failed step or evaluate_only returns model[g] bit for bit.  A
 *      group without members gets status 1, inliers 0, chi2 0, views 0.  views[g]: the member views with a count > 0.
 *      pose_out (optional) [B,3,4]: the compose rule applied to cam and model_out (model with evaluate_only and no model_out), written
 *      for every member view.  member and group_start are device arrays: every start, end (start <= end <= B) and member index is
 *      clamped into range before use.
 *      With one view per group and every cam exactly [I|0], model_out, status, inliers and chi2 are tp_joint_align_step's on the same
 *      terms bit for bit, and with one term at weight 1 that term's own step's.
 *      Launches: each present term's own (as K33), then view_sums (grid B x 64: gather, weight, transform, one 32-double record per
 *      view into the workspace), group_solve (grid Gr x 64) and, with pose_out, the compose (grid Gr x 64 over the members).  No
 *      atomics, no allocation, no host synchronisation; bit-identical from run to run.  Safe to capture.
 *      Refused (-1, tp_last_error) before anything is launched: K33's list (null args; no term, or none with a weight > 0; a bad
 *      weight or damping; B outside 1 .. 65535; a term whose B differs, or whose H, W or intr differs from another's; two terms
 *      sharing a workspace; whatever a term's own step refuses) and: Gr outside 1 .. B; null cam, pose, model, member, group_start,
 *      status, inliers, chi2, views or workspace; a workspace that is not 16-byte aligned; model_out missing without evaluate_only, or
 *      overlapping model; pose_out overlapping pose or cam; a present term whose pose is not args' pose; the multi-view workspace
 *      overlapping a term's.  tp_pose_compose refuses null pointers, B outside 1 .. 2^24, Gr < 1 and an out overlapping cam or model.
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_pose_compose_args {
  int B, Gr;
  const float* cam;          /* [B,3,4] world -> camera */
  const float* model;        /* [Gr,3,4] model -> world */
  const int32_t* group;      /* [B] the model of each view; clamped into 0 .. Gr-1 */
  float* out;                /* [B,3,4] out: cam[i] o model[group[i]] */
} tp_pose_compose_args;
int tp_pose_compose(const tp_pose_compose_args* args, tp_stream_t stream);

typedef struct tp_multiview_args {
  int B, Gr;
  const float* cam;          /* [B,3,4] world -> camera of each view */
  const float* pose;         /* [B,3,4] the composed poses every term's planes were rendered at (each term's pose must be this pointer) */
  const float* model;        /* [Gr,3,4] the current model -> world poses */
  const int32_t* member;     /* [B] view indices, the groups one after the other, ascending inside a group; clamped */
  const int32_t* group_start; /* [Gr+1] group g owns member[group_start[g] .. group_start[g+1] - 1]; clamped */
  float w_sil, w_photo, w_icp; /* finite, >= 0: K33's weights */
  float damping;             /* finite, >= 0 */
  int evaluate_only;         /* non-zero: inliers, chi2, status and views of model; no step */
  float* model_out;          /* [Gr,3,4] out; may be NULL with evaluate_only; must not overlap model */
  float* pose_out;           /* [B,3,4] out or NULL: cam o model_out per member view; must not overlap pose or cam */
  int32_t* status;           /* [Gr] out: 0 ok, 1 fewer than 6 kept pixels in the whole group, 3 not positive definite */
  int32_t* inliers;          /* [Gr] out */
  float* chi2;               /* [Gr] out */
  int32_t* views;            /* [Gr] out: member views with a count > 0 */
  void* workspace;           /* tp_multiview_workspace_bytes(B) bytes, 16-byte aligned; needs no clearing */
} tp_multiview_args;
size_t tp_multiview_workspace_bytes(int B);  /* 256 * B; 0 for a non-positive B */
int tp_multiview_align_step(const tp_multiview_args* mv,
                            const tp_silhouette_align_args* sil,   /* may be NULL */
                            const tp_photo_align_args* photo,      /* may be NULL */
                            const tp_depth_icp_args* icp,          /* may be NULL */
                            tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K40  per-image, per-channel FIRST-ORDER SPHERICAL-HARMONIC shading (ambient + directional) and a bias between a rendering and its
 *      photograph (texpose_amd/ops/refine.py: photo_lighting; restated in tests/photo_lighting_ref.py; the project's own step, no
 *      reference code).  K37's sibling for a light that has a direction: face / zbuf / rgb are K19's planes of the
 *      mesh (verts, faces) at `pose`; the call fits  o_k ~ (l0_k + l1_k n_x + l2_k n_y + l3_k n_z) c_k + beta_k  per image b and
 *      channel k by least squares over the pixels the light that came in (light_in [B,3,5]: per channel (l0, l1, l2, l3, beta); NULL:
 *      (1, 0, 0, 0, 0)) explains within tau, n the unit normal of the pixel's FACE in the camera frame, turned towards the camera; where
 *      rgb_out is given it applies the new light to the rendering.  The model contains K37's (l1 = l2 = l3 = 0).
 *      Per pixel (row i, column j) of image b, with fr as K37 (frame CLAMPED into [0, Ft)), everything in fp64 from the fp32 inputs,
 *      evaluated as written (no contraction):
 *        1.-4. K37's steps 1 - 4: interior, z = zbuf[b,i,j] > 0 and finite, mask[fr,i,j] != 0, the six colours c_k, o_k finite
 *        5. f = face[b,i,j];  skipped unless 0 <= f < F and all three of faces[f] lie in [0, V)       (nothing is read out of bounds)
 *        6. v0, v1, v2 = verts[faces[f]];  m = (v1 - v0) x (v2 - v0);  [R|t] = pose[b];
 *           n_r = (R[r][0] m_x + R[r][1] m_y) + R[r][2] m_z;   d = (n_x n_x + n_y n_y) + n_z n_z;   skipped unless d is finite and > 0;
 *           n = n / sqrt(d)   (a division per component)
 *        7. x_r = ((R[r][0] v0_x + R[r][1] v0_y) + R[r][2] v0_z) + t_r;   if (n_x x_x + n_y x_y) + n_z x_z > 0 then n = -n
 *        8. per channel the regressors x = (c, c n_x, c n_y, c n_z, 1): entry 0 is c itself
 *        9. with (l, beta) = light_in[b,k]:  p_k = (((l0 x_0 + l1 x_1) + l2 x_2) + l3 x_3) + beta;  r_k = o_k - p_k;
 *           kept iff (r_0^2 + r_1^2) + r_2^2 <= tau * tau
 *      Steps 5 - 7 are the pixel's VALID NORMAL (they read neither colours nor the mask); K19's normal plane is not used.
 *      64 sums over the kept pixels: [0] n (+ 1 per pixel) and, for channel k, [1 + 21 k ..]: the 15 products x_i x_j, j >= i,
 *      row-major, the 5 products x_i o, and o o.  K30's / K37's order: a thread owns four consecutive flat pixels (ascending), a
 *      workgroup 1024; butterfly sums inside a wave, the four waves in ascending order, one 64-double record per workgroup, the
 *      records of an image in ascending order.  No atomics; the outputs are a function of the inputs alone, bit-identical from run
 *      to run and under graph replay.
 *      Per image and channel, in fp64 as written, A the 5 x 5 matrix of the 15 sums, r the 5, Soo the last:
 *        Cholesky of A with K29's pivot rule (a pivot must be finite, > 1e-10 x its diagonal entry and > 0), L y = r, L^T x = y, every
 *        inner sum in ascending index order starting from the entry itself.  x is ACCEPTED iff the factorisation passes, all five
 *        values are finite, gain_min <= x_0 <= gain_max and sqrt((x_1^2 + x_2^2) + x_3^2) <= x_0 (the shading is non-negative for
 *        every normal).  Otherwise K37's closed form on the sub-sums Sc = A[0][4], So = r[4], Scc = A[0][0], Sco = r[0] (and n):
 *        mc, mo, var, cov, the clamp, the flat rule and b = mo - g mc exactly as K37 states them, x = (g, 0, 0, 0, b), and
 *        TP_LIGHTING_FALLBACK << k is set in flags beside K37's TP_EXPOSURE_CLAMPED << k / TP_EXPOSURE_FLAT << k; where the kept sets
 *        agree g and b are K37's bit for bit.
 *        xr = (((x_0 r_0 + x_1 r_1) + x_2 r_2) + x_3 r_3) + x_4 r_4;  (Ax)_i likewise over row i;  xAx likewise over x_i (Ax)_i;
 *        sse_k = (Soo - 2 xr) + xAx
 *      count = n;  rms = sqrt(max(0, (sse_0 + sse_1) + sse_2) / n) (NaN at n = 0);  status = 1 where n < 6; else 3 where one of the 15
 *      coefficients or rms rounded to fp32 is not finite; else 0.  light = the 15 coefficients rounded to fp32 where status == 0;
 *      otherwise light_in bit for bit ((1, 0, 0, 0, 0) where NULL).  flags are those of the fit just made whatever the status.
 *      Apply, where rgb_out is given: a pixel with zbuf > 0 and finite (border pixels included) becomes
 *        s = ((l0 + l1 n_x) + l2 n_y) + l3 n_z   in fp64 from the fp32 light just written and the pixel's valid normal, rounded to fp32
 *            ONCE; s = l0 itself where the pixel has no valid normal
 *        rgb_out[b,i,j,k] = s * rgb[b,i,j,k] + beta   as two fp32 operations (a product, then a sum)
 *      so a light without a directional part gives K37's apply bit for bit.  Every other pixel is copied bit for bit, and with
 *      rgb_out == rgb is not written.
 *      Three launches on the stream (reduce, solve, apply; two without rgb_out).  Refused (-1, tp_last_error) before anything is
 *      launched: K37's list (sizes, Ft without frame, tau, gain_min / gain_max, min_var, null pointers, workspace alignment, an rgb_out
 *      overlapping rgb without being rgb, light overlapping light_in) and null verts, faces, face or pose and V <= 0 or F <= 0.
 *      No input value causes an access out of bounds: frame is clamped, face and the vertex indices are checked before use.  No
 *      allocation, no host synchronisation; outputs and workspace must not overlap inputs otherwise.  Safe to capture.
 *      Left out: second-order SH, interpolated vertex normals, shadows and speculars, a light shared by the views of a group,
 *      eliminating the light inside the pose step's system, a ridge term (DESIGN section 30 says why none was needed).
 * ------------------------------------------------------------------------------------------ */
#define TP_LIGHTING_FALLBACK 64  /* flags: << k, channel k took K37's closed form (with its TP_EXPOSURE_CLAMPED / TP_EXPOSURE_FLAT << k) */
typedef struct tp_photo_lighting_args {
  const float* verts;        /* [V,3] */
  const int32_t* faces;      /* [F,3]; a face with an index outside [0, V) has no normal */
  const int32_t* face;       /* [B,H,W] K19's face index at the current poses; outside [0, F): no normal */
  const float* zbuf;         /* [B,H,W] K19's depth at the current poses: <= 0 or NaN: background */
  const float* rgb;          /* [B,H,W,3] K19's colours at the current poses */
  const float* pose;         /* [B,3,4] the poses the planes were rendered at */
  const float* image;        /* [Ft,H,W,3] the photograph, channels last */
  const int32_t* frame;      /* [B] index into image (and mask), or NULL: b when Ft == B, 0 when Ft == 1 */
  const uint8_t* mask;       /* [Ft,H,W] or NULL; 0: the pixel is skipped */
  const float* light_in;     /* [B,3,5] or NULL ((1, 0, 0, 0, 0)): the light the keep rule judges by */
  int V, F, B, Ft, H, W;
  float tau;                 /* finite, > 0 */
  float gain_min, gain_max;  /* 0 < gain_min <= 1 <= gain_max, finite: the range of l0 */
  float min_var;             /* finite, >= 0: K37's, for a channel that falls back */
  float* light;              /* [B,3,5] out; must not overlap light_in */
  int32_t* count;            /* [B] out */
  float* rms;                /* [B] out, colour units */
  int32_t* status;           /* [B] out: 0 ok, 1 fewer than 6 kept pixels, 3 not finite */
  int32_t* flags;            /* [B] out: TP_LIGHTING_FALLBACK << k | TP_EXPOSURE_CLAMPED << k | TP_EXPOSURE_FLAT << k */
  float* rgb_out;            /* [B,H,W,3] out, rgb itself (in place) or NULL (fit only) */
  void* workspace;           /* tp_photo_lighting_workspace_bytes(B, H, W) bytes, 16-byte aligned; needs no clearing */
} tp_photo_lighting_args;
size_t tp_photo_lighting_workspace_bytes(int B, int H, int W);  /* 512 * B * ceil(H * W / 1024); 0 for non-positive sizes */
int tp_photo_lighting(const tp_photo_lighting_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K41  the per-pixel step between K35's shading and K36's adjoint when face texels are fitted as an ALBEDO under one first-order SH
 *      light per view (texpose_amd/ops/scene.py: face_texel_light; texpose_amd/face_texels.py: FaceTexelFitter(lighting=True); restated
 *      in tests/face_texel_light_ref.py; the project's own step, no reference code).  The fitter minimises
 *        sum_b sum_p m_p | s_b(n_p) * (S x)_p + beta_b - I_p |^2 + lam |x - prior|^2
 *      over the node colours x and the lights; with the lights fixed its normal equations are (S^T D S + lam) x = S^T m s (I - beta) +
 *      lam prior with D = m s^2, and this call turns S x (or S p) into what the adjoint consumes.  face is K19's plane of the mesh
 *      (verts, faces) at `pose`, light [B,3,5] per channel (l0, l1, l2, l3, beta) as K40 writes it, colour [B,H,W,3] K35's shading.
 *      Per pixel p of image b and channel k:
 *        covered iff 0 <= face < F;  m = weight[p] (1 where weight is NULL)
 *        the pixel is OFF -- and writes +0 to grad and diag and adds nothing to the sums -- where it is not covered, where m is not
 *        finite or m <= 0, and where one of its three colours (or, in residual mode, of its three image values) is not finite
 *        s_k = K40's apply shading: ((l0 + l1 n_x) + l2 n_y) + l3 n_z in fp64 from the fp32 light and the pixel's VALID NORMAL (K40's
 *              steps 5 - 7), rounded to fp32 ONCE; l0 itself where the pixel has no valid normal
 *        everything below is fp32, one rounding per operation, evaluated as written (no contraction):
 *        a_k = m * s_k
 *        residual mode (image given):  q_k = s_k * c_k;  p_k = q_k + beta_k  (K40's two operations: p is its applied rendering bit
 *                                      for bit);  e_k = I_k - p_k;  grad_k = a_k * e_k
 *        operator mode (image NULL):   q_k = s_k * c_k;  grad_k = a_k * q_k
 *        diag_k = a_k * s_k   (where diag is given: the diagonal D of the operator; one adjoint of it is the preconditioner)
 *      Every pixel of grad (and diag) is written: the outputs need no clearing and are a function of the inputs alone.
 *      sums [B,2] (residual mode only): [0] the sum over the pixels that are on of (double)m * (((double)e_0 e_0 + (double)e_1 e_1) +
 *      (double)e_2 e_2), [1] the sum of (double)m, in fp64 in K30's order: a thread owns four consecutive flat pixels (ascending), a
 *      workgroup 1024; butterfly sums inside a wave, the four waves in ascending order, one record of two doubles per (image, tile)
 *      in the workspace, and a second kernel that adds an image's records in ascending tile order.  No atomics: bit-identical from
 *      run to run and under graph replay.
 *      One launch on the stream, two with sums.  Refused (-1, tp_last_error) before anything is launched: a non-positive size, B >
 *      65535, H * W >= 2^31, a null verts, faces, face, pose, light, colour or grad, sums without image, sums without a workspace or
 *      with one that is not 8-byte aligned, and an output (grad, diag, sums, the workspace) that overlaps an input or another output.
 *      No input value causes an access out of bounds: face and the vertex indices are checked before use as in K40.  No allocation,
 *      no host synchronisation.  Safe to capture.
 *      Left out: the shading fused into K35 / K36 themselves, one light for several views, second-order SH, a robust loss.
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_face_texel_light_args {
  const float* verts;        /* [V,3] */
  const int32_t* faces;      /* [F,3]; a face with an index outside [0, V) has no normal */
  const int32_t* face;       /* [B,H,W] K19's face plane (any values); outside [0, F): not covered */
  const float* pose;         /* [B,3,4] the poses the plane was rendered at */
  const float* light;        /* [B,3,5] per channel (l0, l1, l2, l3, beta) */
  const float* colour;       /* [B,H,W,3] S x (residual mode) or S p (operator mode) */
  const float* image;        /* [B,H,W,3] the photographs, or NULL: operator mode */
  const float* weight;       /* [B,H,W] m, or NULL: 1 */
  int V, F, B, H, W;
  float* grad;               /* [B,H,W,3] out */
  float* diag;               /* [B,H,W,3] out or NULL */
  double* sums;              /* [B,2] out or NULL; residual mode only */
  void* workspace;           /* with sums: tp_face_texel_light_workspace_bytes(B, H, W) bytes, 8-byte aligned; needs no clearing */
} tp_face_texel_light_args;
size_t tp_face_texel_light_workspace_bytes(int B, int H, int W);  /* 16 * B * ceil(H * W / 1024); 0 for non-positive sizes */
int tp_face_texel_light(const tp_face_texel_light_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K42  robust (IRLS) weights of a photometric residual, scaled per image by an EXACT median found on the device (texpose_amd/ops/
 *      scene.py: robust_weight; texpose_amd/face_texels.py: FaceTexelFitter(robust=...); restated in tests/robust_weight_ref.py; the
 *      project's own step, no reference code).  model and image are [B,H,W,3] fp32, weight [B,H,W] the base weight
 *      (NULL: 1 everywhere).  Per pixel p of image b, evaluated as written (no contraction):
 *        1. e_k = (double)image_k - (double)model_k;  q = (float)(((e_0 e_0 + e_1 e_1) + e_2 e_2) / 3.0): fp64, rounded once.
 *        2. the pixel is COUNTED iff its base weight is finite and > 0, its six colour values are finite and q is finite.  A pixel
 *           that is not counted gets out = +0.
 *        3. count[b] = n, the number of counted pixels; median_q[b] = the exact LOWER median of q over them: the element of rank
 *           (n - 1) / 2 (integer division, 0-based, ascending); 0 for n = 0.
 *        4. s2 = fmax((1.4826 * 1.4826) * (double)median_q[b], (double)sigma_min * sigma_min);  with scale_in given:
 *           s2 = fmax((double)scale_in[b] * scale_in[b], (double)sigma_min * sigma_min), the median is not computed and median_q[b] =
 *           0.  scale[b] = (float)sqrt(s2), for reporting.
 *        5. u2 = (double)q / (((double)c * c) * s2);
 *           TP_ROBUST_TUKEY: w = u2 < 1 ? (1 - u2) * (1 - u2) : 0        (no square root: comparable bit for bit)
 *           TP_ROBUST_HUBER: w = u2 <= 1 ? 1 : 1 / sqrt(u2)
 *           out = (float)((double)base * w)
 *      The median without a sort and without float atomics: q >= 0, and the bit pattern of a non-negative fp32 is monotone in its
 *      value, so a three-level radix select on the bits (the upper 11, the next 11, the last 10) finds the element of the rank
 *      exactly.  The first pass forms q, stores its bits in the workspace (all ones for a pixel that is not counted) and counts the
 *      upper 11 bits; the second and third pass read the stored bits and count the next digit of the keys that carry the prefix found
 *      so far.  Each pass counts into a histogram in LDS per workgroup and adds its non-zero bins to the image's histogram with
 *      INTEGER atomics: sums of integers do not depend on the order of arrival.  One small launch per level (one workgroup per
 *      image) scans the histogram for the bin that holds the rank.  Every output is a function of the inputs alone: bit-identical
 *      from run to run and under graph replay.
 *      Eight launches on the stream (clear, 3 x (count, search), weight); two with scale_in (clear, weight: q is formed in the weight
 *      pass and count[b] is added up with integer atomics).  The workspace needs no clearing.  Refused (-1, tp_last_error) before
 *      anything is launched: a non-positive size, B > 65535, H * W >= 2^31, a null model, image, out, median_q, scale or count, an
 *      unknown kind, c or sigma_min not finite or <= 0, without scale_in a null workspace or one that is not 16-byte aligned, and an
 *      output (out, median_q, scale, count, the workspace) that overlaps an input or another output.  No input value causes an access
 *      out of bounds.  No allocation, no host synchronisation.  Safe to capture.
 *      Left out: a median of the absolute residual per channel, a scale shared between images, other rho functions (Cauchy, Welsch).
 * ------------------------------------------------------------------------------------------ */
enum { TP_ROBUST_TUKEY = 0, TP_ROBUST_HUBER = 1 };
typedef struct tp_robust_weight_args {
  const float* model;        /* [B,H,W,3] the rendering (S x) */
  const float* image;        /* [B,H,W,3] the photographs */
  const float* weight;       /* [B,H,W] base weight, or NULL: 1 */
  const float* scale_in;     /* [B] sigma per image, or NULL: 1.4826 * sqrt(median q) */
  int B, H, W;
  int kind;                  /* TP_ROBUST_TUKEY or TP_ROBUST_HUBER */
  float c;                   /* the tuning constant, in units of sigma: 4.685 (Tukey), 1.345 (Huber) are the usual ones */
  float sigma_min;           /* the floor of sigma: 1 / 255 is one step of an 8-bit photograph */
  float* out;                /* [B,H,W] out: base weight * robust weight */
  float* median_q;           /* [B] out */
  float* scale;              /* [B] out: sigma */
  int32_t* count;            /* [B] out: counted pixels */
  void* workspace;           /* without scale_in: tp_robust_weight_workspace_bytes(B, H, W) bytes, 16-byte aligned; needs no clearing */
} tp_robust_weight_args;
size_t tp_robust_weight_workspace_bytes(int B, int H, int W);  /* 4 * B * H * W rounded up to 16, + 20512 * B; 0 for non-positive sizes */
int tp_robust_weight(const tp_robust_weight_args* args, tp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K43  mip levels of a face-texel texture: a minification filter for K35's shading (texpose_amd/face_texels.py: mip_slots, build_mips,
 *      TexelMips; texpose_amd/ops/scene.py: face_texel_mip_reduce, face_texel_shade_mip; restated in tests/face_texel_mip_ref.py; the
 *      project's own step, no reference code).
 *      The chain.  Level 0 is K35's texture [F, T(R), 3].  Level l has resolution R_l = R >> l and exists while R_(l-1) is even: L
 *      levels need R % 2^(L-1) == 0.  Coarse node (I, J) of a face is fine node (2I, 2J) of the same face; every other fine node is
 *      the midpoint of one coarse lattice edge.  The chain is ONE packed fp32 buffer: level l is a contiguous [F, T(R_l), 3] block at
 *      element offset 3 F sum_{k<l} T(R_k); tp_face_texel_mip_elems(F, R, L) is its size in elements (0 for F <= 0, R outside 1 ..
 *      TP_FACE_TEXEL_MAX_R, L < 1, R % 2^(L-1) != 0 or F sum T(R_k) >= 2^31).
 *
 * K43a tp_face_texel_mip_reduce: one level down, Rf (even) -> Rc = Rf / 2.  The filter is the normalised transpose of linear
 *      prolongation (full weighting on the triangular lattice), written per coarse CELL so that it needs no valence and is the same
 *      rule at mesh vertices, edges and open boundaries.  The slots (f Tc + n, Tc = T(Rc)) that name one unique node u of the coarse
 *      grid come as a CSR pair: slot_list[slot_ptr[u] .. slot_ptr[u+1] - 1] (face_texels.mip_slots builds it from subdivide's
 *      node_index by a stable argsort, so that the slots of a node ascend).  For node u, acc[3] = 0 and wacc = 0 in fp64; for every
 *      slot s = f Tc + n of u in list order, n decoded to (I, J), the six directions d_0 .. d_5 = (1,0), (0,1), (-1,1), (-1,0), (0,-1),
 *      (1,-1), and k = 0 .. 5 in order: where both (I,J) + d_k and (I,J) + d_((k+1)%6) are nodes of the coarse grid (i, j >= 0, i + j
 *      <= Rc) the pair is a coarse cell of f at this corner, and per channel
 *        acc  = acc + ((2 x(2I,2J) + 3 x((2I,2J) + d_k)) + 3 x((2I,2J) + d_((k+1)%6))),   wacc = wacc + 8,
 *      x face f's OWN fine texels (fp32 -> fp64), every product and sum fp64 as written.  The value (float)(acc / wacc) is written to
 *      every slot of u.  On a closed manifold that is x_c / 4 + 3/4 of the mean of the incident edge midpoints, whatever the valence;
 *      a constant texture comes back bit for bit; a non-finite texel propagates.  Entries of slot_list outside 0 .. F Tc - 1 are
 *      skipped and never dereferenced, and a range of slot_ptr is cut to 0 .. F Tc; a node without a valid slot writes nothing.  The
 *      call first clears `coarse` (one asynchronous memset), then one launch, one thread per unique node: no atomics, no float
 *      reduction across threads, no workspace, no host synchronisation; the output is a function of the inputs alone (for a slot_list
 *      that names every slot at most once).  Safe to capture.  Refused (-1, tp_last_error), nothing launched: null pointers, F <= 0,
 *      U <= 0, Rf odd or outside 2 .. TP_FACE_TEXEL_MAX_R, F T(Rf) >= 2^31.
 *
 * K43b tp_face_texel_shade_mip: K35 with a level chosen and blended per pixel.  Arguments as K35, with `mips` (the packed chain) in
 *      the place of texels, L its number of levels, and footprint, finite and > 0: a multiplier on the texel density (an LOD bias of
 *      log2(footprint) / 2; 1 is the rule as derived).  Per pixel: K35's step 1 gives w_0, w_1, w_2 (once; the SAME device function as
 *      K35, texpose_amd/csrc/face_texel_cell.h) and, from the values it has formed already,
 *        d = (((double)footprint (double)(R R)) |(iz_0 iz_1) iz_2|) / (|area| ((|S| |S|) |S|)),   iz_k = 1 / z_k, S = (t_0 + t_1) + t_2
 *      before the clamp: the texel cells of level 0 per pixel, the determinant of d(R w_1, R w_2) / d(px, py) -- 1 / area for the
 *      screen barycentrics times iz_0 iz_1 iz_2 / S^3 for the perspective map.  Level selection, without a transcendental:
 *        d <= 1, L = 1 or d not finite:  level 0 alone; only level 0 is read and the colour is K35's expression exactly;
 *        otherwise e = ilogb(d), l0 = min(e >> 1, L - 1);   l0 = L - 1:  level L - 1 alone;
 *        otherwise t = (ldexp(d, -2 l0) - 1) / 3  (an exact scaling, one subtraction, one division; 0 <= t < 1);  t = 0: level l0
 *        alone; else c = (1 - t) c_l0 + t c_(l0+1) per channel in fp64.
 *      Each c_l is K35's step 2 and three-product sum on level l's texels at R_l under the same w.  Rounded to fp32 once.  The zero
 *      rules and out-of-bounds guarantees are K35's; a non-finite colour at a level that is read gives zero.  One launch, one thread
 *      per pixel, 256 per workgroup, K35's grid; no LDS, no atomics, no workspace, no host synchronisation; safe to capture.
 *      Refused: everything K35 refuses, tp_face_texel_mip_elems(F, R, L) == 0 and a footprint that is not finite or <= 0.
 *      Left out: the adjoint of the mip shade and the refiners / the fitter's forward on it, an anisotropic footprint (the area
 *      measure under-filters at grazing angles), one R per face.
 * ------------------------------------------------------------------------------------------ */
typedef struct tp_face_texel_mip_reduce_args {
  const float* fine;         /* [F,T(Rf),3] */
  const int32_t* slot_ptr;   /* [U+1] */
  const int32_t* slot_list;  /* [F*T(Rf/2)] (any values: entries outside 0 .. F*T(Rf/2)-1 are skipped) */
  int F, Rf, U;
  float* coarse;             /* [F,T(Rf/2),3] out; cleared by the call */
} tp_face_texel_mip_reduce_args;
typedef struct tp_face_texel_shade_mip_args {
  const float* verts;        /* [V,3] as K35 */
  const int32_t* faces;      /* [F,3] */
  const float* mips;         /* the packed chain: tp_face_texel_mip_elems(F, R, L) floats */
  const float* pose;         /* [B,3,4] */
  const float* intr;         /* [B,3,3] */
  const int32_t* face;       /* [B,H,W] K19's face plane (any values) */
  int B, H, W, V, F, R, L;
  float footprint;           /* finite, > 0; 1: the rule as derived */
  float* rgb;                /* [B,H,W,3] out */
} tp_face_texel_shade_mip_args;
int64_t tp_face_texel_mip_elems(int F, int R, int L);     /* 3 F sum_{l<L} T(R >> l); 0 for anything refused */
int tp_face_texel_mip_reduce(const tp_face_texel_mip_reduce_args* args, tp_stream_t stream);
int tp_face_texel_shade_mip(const tp_face_texel_shade_mip_args* args, tp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TEXPOSE_AMD_H */
