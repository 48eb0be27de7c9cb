// K19  hard mesh rasteriser for the surfel maps of the adaptation loops (rgbsyn / nocs / normal files)
// ref: compute_surfelinfo.py:37-56,100-140 (normal_from_depth + the colour / NOCS renders), tools/mvrenderer.py:33-180,695-730
//      (MVRenderer with faces_per_pixel = 1), compute_box.py:41-60 (the rays of normal_from_depth).
//
// Three launches on one stream, no allocation, no host synchronisation:
//   1. face setup, one thread per (image, face): [R|t], K, screen positions in fp64; bounding box in pixel indices and the three
//      barycentric planes b_k(j, i) = A_k (j - j0) + B_k (i - i0) + C_k, anchored at the box's first pixel (j0, i0) so that the fp32
//      evaluation never cancels image-sized terms; per-vertex 1/z.  64 bytes per record in the workspace.
//   2. raster, one workgroup per 16x16-pixel tile per image: chunks of 256 face boxes are culled against the tile, the survivors are
//      compacted into LDS by wave ballots and tested at the pixel centres.  Each pixel keeps the minimum of the 64-bit key
//      (bits of z, face index): the winner does not depend on the order faces arrive in, and no atomics are needed.  Shading of the
//      winner (perspective-correct vertex colour and NOCS) follows in the same kernel.
//   3. normals from the depth map, one thread per pixel, in fp64 (compute_surfelinfo.normal_from_depth, see normal_kernel).
//
// K34  tp_mesh_raster_culled: the same planes, bit for bit, with one launch more.  Between 1 and 2 chunk_box_kernel stores the union of
//      the pixel boxes of every chunk of 256 face records; raster_culled_kernel tests a tile against that one box before it enters the
//      chunk.  A pixel's key minimum is taken over a superset of the faces whose boxes hold it, so skipping a chunk whose union box
//      misses the tile removes only faces that could not have entered the minimum: no output bit changes.
#include "tp_common.h"

namespace {

constexpr int kTile = 16;
constexpr int kChunk = kTile * kTile;   // faces per LDS chunk = threads per workgroup
constexpr int kRecFloats = 16;           // one face record: bbox (4 x int32), b-planes (9), 1/z (3)

struct RasterParams {
  const float* verts; const int32_t* faces; const float* vcolor;
  float nocs_center[3], nocs_scale[3];
  const float* pose; const float* intr;
  int B, H, W, V, F;
  float* zbuf; int32_t* face; float* rgb; float* nocs; float* normal;
  float4* rec;                             // [B, F] x 4 float4
};

// ---- 1. face setup -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) face_setup_kernel(RasterParams p) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)p.B * p.F) return;
  const int b = (int)(gid / p.F), f = (int)(gid - (int64_t)b * p.F);
  const float* P = p.pose + 12 * b;
  const float* K = p.intr + 9 * b;
  int4 box = make_int4(INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN);   // never overlaps a tile
  float coef[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  bool ok = true;
  double u[3], v[3], iz[3];
  for (int k = 0; k < 3; ++k) {
    const int vi = p.faces[3 * (int64_t)f + k];
    if (vi < 0 || vi >= p.V) { ok = false; break; }
    const double X = p.verts[3 * (int64_t)vi], Y = p.verts[3 * (int64_t)vi + 1], Z = p.verts[3 * (int64_t)vi + 2];
    double c[3];
    for (int r = 0; r < 3; ++r) c[r] = (double)P[4 * r] * X + (double)P[4 * r + 1] * Y + (double)P[4 * r + 2] * Z + (double)P[4 * r + 3];
    // a vertex at or behind the camera plane drops the face (PyTorch3D would rasterise it unclipped: DESIGN.md section 11)
    if (!(c[2] > 0.0) || !isfinite(c[0]) || !isfinite(c[1]) || !isfinite(c[2])) { ok = false; break; }
    const double q0 = (double)K[0] * c[0] + (double)K[1] * c[1] + (double)K[2] * c[2];
    const double q1 = (double)K[3] * c[0] + (double)K[4] * c[1] + (double)K[5] * c[2];
    const double q2 = (double)K[6] * c[0] + (double)K[7] * c[1] + (double)K[8] * c[2];
    u[k] = q0 / q2;
    v[k] = q1 / q2;
    iz[k] = 1.0 / c[2];
  }
  double area = 0.0;
  if (ok) {
    area = (u[1] - u[0]) * (v[2] - v[0]) - (v[1] - v[0]) * (u[2] - u[0]);
    ok = isfinite(area) && fabs(area) > 1e-10;        // degenerate faces are skipped
  }
  if (ok) {
    // pixel (row i, column j) is sampled at (j + 0.5, i + 0.5): the candidates are the centres inside the bounding box
    const double xmin = fmin(u[0], fmin(u[1], u[2])), xmax = fmax(u[0], fmax(u[1], u[2]));
    const double ymin = fmin(v[0], fmin(v[1], v[2])), ymax = fmax(v[0], fmax(v[1], v[2]));
    const double j0 = fmax(ceil(xmin - 0.5), 0.0), j1 = fmin(floor(xmax - 0.5), (double)(p.W - 1));
    const double i0 = fmax(ceil(ymin - 0.5), 0.0), i1 = fmin(floor(ymax - 0.5), (double)(p.H - 1));
    if (j0 <= j1 && i0 <= i1) {
      box = make_int4((int)j0, (int)j1, (int)i0, (int)i1);
      const double px = j0 + 0.5, py = i0 + 0.5, ia = 1.0 / area;
      for (int k = 0; k < 3; ++k) {
        const int s = (k + 1) % 3, e = (k + 2) % 3;     // b_k: the edge opposite vertex k, from vertex s to vertex e
        const double ex = u[e] - u[s], ey = v[e] - v[s];
        coef[3 * k + 0] = (float)(-ey * ia);
        coef[3 * k + 1] = (float)(ex * ia);
        coef[3 * k + 2] = (float)((ex * (py - v[s]) - ey * (px - u[s])) * ia);
        coef[9 + k] = (float)iz[k];
      }
    }
  }
  float4* r = p.rec + 4 * gid;
  r[0] = make_float4(__int_as_float(box.x), __int_as_float(box.y), __int_as_float(box.z), __int_as_float(box.w));
  r[1] = make_float4(coef[0], coef[1], coef[2], coef[3]);
  r[2] = make_float4(coef[4], coef[5], coef[6], coef[7]);
  r[3] = make_float4(coef[8], coef[9], coef[10], coef[11]);
}

// barycentrics of a record at the pixel (j, i); one code path for the depth test and the shading, so both see the same bits
struct Bary { float b0, b1, b2, zinv; };
__device__ __forceinline__ Bary bary_at(const float4& r0, const float4& r1, const float4& r2, const float4& r3, int j, int i) {
  const float dj = (float)(j - __float_as_int(r0.x)), di = (float)(i - __float_as_int(r0.z));
  Bary o;
  o.b0 = __fmaf_rn(r1.x, dj, __fmaf_rn(r1.y, di, r1.z));
  o.b1 = __fmaf_rn(r1.w, dj, __fmaf_rn(r2.x, di, r2.y));
  o.b2 = __fmaf_rn(r2.z, dj, __fmaf_rn(r2.w, di, r3.x));
  o.zinv = __fmaf_rn(o.b2, r3.w, __fmaf_rn(o.b1, r3.z, __fmul_rn(o.b0, r3.y)));
  return o;
}

// ---- 2. raster + shading --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kChunk) raster_kernel(RasterParams p, int tiles_x) {
  __shared__ float4 s_rec[kChunk][4];
  __shared__ int s_wave_count[kChunk / tp::kWave];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const int tx0 = (blockIdx.x % tiles_x) * kTile, ty0 = (blockIdx.x / tiles_x) * kTile;
  const int tx1 = min(tx0 + kTile, p.W) - 1, ty1 = min(ty0 + kTile, p.H) - 1;
  const int j = tx0 + (tid % kTile), i = ty0 + (tid / kTile);
  const float4* rec = p.rec + 4 * (int64_t)b * p.F;
  unsigned long long best = ~0ull;
  for (int base = 0; base < p.F; base += kChunk) {
    const int f = base + tid;
    bool keep = false;
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (f < p.F) {
      r0 = rec[4 * (int64_t)f];
      keep = __float_as_int(r0.x) <= tx1 && __float_as_int(r0.y) >= tx0 && __float_as_int(r0.z) <= ty1 && __float_as_int(r0.w) >= ty0;
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave_count[wave] = __popcll(m);
    __syncthreads();
    int off = 0, n = 0;
#pragma unroll
    for (int w = 0; w < kChunk / tp::kWave; ++w) {
      const int c = s_wave_count[w];
      off += (w < wave) ? c : 0;
      n += c;
    }
    if (keep) {
      const int slot = off + __popcll(m & ((1ull << lane) - 1ull));
      r0.y = __int_as_float(f);                          // the face index rides in the (already tested) jmax word
      s_rec[slot][0] = r0;
      s_rec[slot][1] = rec[4 * (int64_t)f + 1];
      s_rec[slot][2] = rec[4 * (int64_t)f + 2];
      s_rec[slot][3] = rec[4 * (int64_t)f + 3];
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      const float4 r0k = s_rec[k][0], r1 = s_rec[k][1], r2 = s_rec[k][2], r3 = s_rec[k][3];
      const Bary q = bary_at(r0k, r1, r2, r3, j, i);
      if (q.b0 > 0.f && q.b1 > 0.f && q.b2 > 0.f) {
        const float z = __fdiv_rn(1.0f, q.zinv);
        if (z > 1e-8f && z < INFINITY) {
          const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)__float_as_int(r0k.y);
          best = key < best ? key : best;
        }
      }
    }
    __syncthreads();
  }
  if (j >= p.W || i >= p.H) return;
  const int64_t pix = ((int64_t)b * p.H + i) * p.W + j;
  if (best == ~0ull) {
    p.zbuf[pix] = -1.0f;
    if (p.face) p.face[pix] = -1;
    for (int c = 0; c < 3; ++c) {
      if (p.rgb) p.rgb[3 * pix + c] = 0.0f;
      if (p.nocs) p.nocs[3 * pix + c] = 0.0f;
    }
    return;
  }
  const int f = (int)(best & 0xffffffffu);
  p.zbuf[pix] = __uint_as_float((unsigned)(best >> 32));
  if (p.face) p.face[pix] = f;
  if (!p.rgb && !p.nocs) return;
  const float4* r = rec + 4 * (int64_t)f;
  const float4 r3 = r[3];
  const Bary q = bary_at(r[0], r[1], r[2], r3, j, i);
  // perspective-corrected barycentrics (b_k / z_k) / sum_m (b_m / z_m)
  const float w0 = __fdiv_rn(__fmul_rn(q.b0, r3.y), q.zinv), w1 = __fdiv_rn(__fmul_rn(q.b1, r3.z), q.zinv);
  const float w2 = __fdiv_rn(__fmul_rn(q.b2, r3.w), q.zinv);
  const int v0 = p.faces[3 * (int64_t)f], v1 = p.faces[3 * (int64_t)f + 1], v2 = p.faces[3 * (int64_t)f + 2];
  for (int c = 0; c < 3; ++c) {
    if (p.rgb) {
      const float a0 = p.vcolor[3 * (int64_t)v0 + c], a1 = p.vcolor[3 * (int64_t)v1 + c], a2 = p.vcolor[3 * (int64_t)v2 + c];
      p.rgb[3 * pix + c] = __fmaf_rn(w2, a2, __fmaf_rn(w1, a1, __fmul_rn(w0, a0)));
    }
    if (p.nocs) {
      // mvrenderer.py:702-716: ((x - mean) / max|x - mean| + 1) / 2 per vertex, then interpolated
      const float ct = p.nocs_center[c], sc = p.nocs_scale[c];
      const float a0 = __fmul_rn(__fadd_rn(__fdiv_rn(__fsub_rn(p.verts[3 * (int64_t)v0 + c], ct), sc), 1.0f), 0.5f);
      const float a1 = __fmul_rn(__fadd_rn(__fdiv_rn(__fsub_rn(p.verts[3 * (int64_t)v1 + c], ct), sc), 1.0f), 0.5f);
      const float a2 = __fmul_rn(__fadd_rn(__fdiv_rn(__fsub_rn(p.verts[3 * (int64_t)v2 + c], ct), sc), 1.0f), 0.5f);
      p.nocs[3 * pix + c] = __fmaf_rn(w2, a2, __fmaf_rn(w1, a1, __fmul_rn(w0, a0)));
    }
  }
}

// ---- K34: chunk boxes + the culled raster ---------------------------------------------------------------------------------------
// The body of raster_kernel's chunk loop and its epilogue as functions for raster_culled_kernel: the same tests and the same rounded
// operations per face, so the same keys.  raster_kernel above keeps its own text, so the parent's kernel compiles from unchanged
// source.  Two things differ in how the chunk body WAITS, not in what it computes: a tile that enters few chunks gets nothing from
// other tiles' loads, so (1) word 0 of the chunk's records comes from the caller, who loads the next surviving chunk's before this
// one is processed (one dependent round of loads per chunk instead of two), and (2) the candidate loop reads record k + 1 from LDS
// before it evaluates record k.
struct TileCtx { int tid, lane, wave, b, tx0, ty0, tx1, ty1, j, i; };

__device__ __forceinline__ TileCtx tile_ctx(const RasterParams& p, int tiles_x) {
  TileCtx t;
  t.tid = threadIdx.x; t.lane = t.tid & 63; t.wave = t.tid >> 6;
  t.b = blockIdx.y;
  t.tx0 = (blockIdx.x % tiles_x) * kTile; t.ty0 = (blockIdx.x / tiles_x) * kTile;
  t.tx1 = min(t.tx0 + kTile, p.W) - 1; t.ty1 = min(t.ty0 + kTile, p.H) - 1;
  t.j = t.tx0 + (t.tid % kTile); t.i = t.ty0 + (t.tid / kTile);
  return t;
}

// word 0 of record base + tid (zeros for f >= F: tested by nobody)
__device__ __forceinline__ float4 chunk_word0(const RasterParams& p, const TileCtx& t, const float4* rec, int base) {
  const int f = base + t.tid;
  return f < p.F ? rec[4 * (int64_t)f] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// one chunk of 256 records from ``base`` on, ``r0`` = chunk_word0(base): box test, ballot compaction into s_rec, the bary_at tests, the
// key minimum.  Every thread of the workgroup calls it with the same ``base`` (three barriers inside).
__device__ __forceinline__ void raster_chunk(const RasterParams& p, const TileCtx& t, const float4* rec, int base, float4 r0, float4 (*s_rec)[4],
                                             int* s_wave_count, unsigned long long& best) {
  const int f = base + t.tid;
  const bool keep = f < p.F && __float_as_int(r0.x) <= t.tx1 && __float_as_int(r0.y) >= t.tx0 && __float_as_int(r0.z) <= t.ty1 &&
                    __float_as_int(r0.w) >= t.ty0;
  const unsigned long long m = __ballot(keep);
  if (t.lane == 0) s_wave_count[t.wave] = __popcll(m);
  __syncthreads();
  int off = 0, n = 0;
#pragma unroll
  for (int w = 0; w < kChunk / tp::kWave; ++w) {
    const int c = s_wave_count[w];
    off += (w < t.wave) ? c : 0;
    n += c;
  }
  if (keep) {
    const int slot = off + __popcll(m & ((1ull << t.lane) - 1ull));
    r0.y = __int_as_float(f);                          // the face index rides in the (already tested) jmax word
    s_rec[slot][0] = r0;
    s_rec[slot][1] = rec[4 * (int64_t)f + 1];
    s_rec[slot][2] = rec[4 * (int64_t)f + 2];
    s_rec[slot][3] = rec[4 * (int64_t)f + 3];
  }
  __syncthreads();
  float4 n0 = s_rec[0][0], n1 = s_rec[0][1], n2 = s_rec[0][2], n3 = s_rec[0][3];      // (n = 0: read and never used)
  for (int k = 0; k < n; ++k) {
    const float4 r0k = n0, r1 = n1, r2 = n2, r3 = n3;
    const int kn = min(k + 1, kChunk - 1);               // the next record, in flight while this one is evaluated (k + 1 = n: unused)
    n0 = s_rec[kn][0]; n1 = s_rec[kn][1]; n2 = s_rec[kn][2]; n3 = s_rec[kn][3];
    const Bary q = bary_at(r0k, r1, r2, r3, t.j, t.i);
    if (q.b0 > 0.f && q.b1 > 0.f && q.b2 > 0.f) {
      const float z = __fdiv_rn(1.0f, q.zinv);
      if (z > 1e-8f && z < INFINITY) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)__float_as_int(r0k.y);
        best = key < best ? key : best;
      }
    }
  }
  __syncthreads();
}

// background values or the winner's planes of pixel (t.j, t.i)
__device__ __forceinline__ void raster_epilogue(const RasterParams& p, const TileCtx& t, const float4* rec, unsigned long long best) {
  const int j = t.j, i = t.i;
  if (j >= p.W || i >= p.H) return;
  const int64_t pix = ((int64_t)t.b * p.H + i) * p.W + j;
  if (best == ~0ull) {
    p.zbuf[pix] = -1.0f;
    if (p.face) p.face[pix] = -1;
    for (int c = 0; c < 3; ++c) {
      if (p.rgb) p.rgb[3 * pix + c] = 0.0f;
      if (p.nocs) p.nocs[3 * pix + c] = 0.0f;
    }
    return;
  }
  const int f = (int)(best & 0xffffffffu);
  p.zbuf[pix] = __uint_as_float((unsigned)(best >> 32));
  if (p.face) p.face[pix] = f;
  if (!p.rgb && !p.nocs) return;
  const float4* r = rec + 4 * (int64_t)f;
  const float4 r3 = r[3];
  const Bary q = bary_at(r[0], r[1], r[2], r3, j, i);
  // perspective-corrected barycentrics (b_k / z_k) / sum_m (b_m / z_m)
  const float w0 = __fdiv_rn(__fmul_rn(q.b0, r3.y), q.zinv), w1 = __fdiv_rn(__fmul_rn(q.b1, r3.z), q.zinv);
  const float w2 = __fdiv_rn(__fmul_rn(q.b2, r3.w), q.zinv);
  const int v0 = p.faces[3 * (int64_t)f], v1 = p.faces[3 * (int64_t)f + 1], v2 = p.faces[3 * (int64_t)f + 2];
  for (int c = 0; c < 3; ++c) {
    if (p.rgb) {
      const float a0 = p.vcolor[3 * (int64_t)v0 + c], a1 = p.vcolor[3 * (int64_t)v1 + c], a2 = p.vcolor[3 * (int64_t)v2 + c];
      p.rgb[3 * pix + c] = __fmaf_rn(w2, a2, __fmaf_rn(w1, a1, __fmul_rn(w0, a0)));
    }
    if (p.nocs) {
      const float ct = p.nocs_center[c], sc = p.nocs_scale[c];
      const float a0 = __fmul_rn(__fadd_rn(__fdiv_rn(__fsub_rn(p.verts[3 * (int64_t)v0 + c], ct), sc), 1.0f), 0.5f);
      const float a1 = __fmul_rn(__fadd_rn(__fdiv_rn(__fsub_rn(p.verts[3 * (int64_t)v1 + c], ct), sc), 1.0f), 0.5f);
      const float a2 = __fmul_rn(__fadd_rn(__fdiv_rn(__fsub_rn(p.verts[3 * (int64_t)v2 + c], ct), sc), 1.0f), 0.5f);
      p.nocs[3 * pix + c] = __fmaf_rn(w2, a2, __fmaf_rn(w1, a1, __fmul_rn(w0, a0)));
    }
  }
}

// chunk c of image b: the union (jmin, jmax, imin, imax) of the boxes of records c * 256 .. c * 256 + 255.  A dropped face holds the
// empty box (INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN), which is also what stands for f >= F and is neutral under min / max.
__global__ void __launch_bounds__(kChunk) chunk_box_kernel(RasterParams p, int4* cbox, int n_chunks) {
  __shared__ int4 s_box[kChunk / tp::kWave];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, f = (int)blockIdx.x * kChunk + tid;
  int4 box = make_int4(INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN);
  if (f < p.F) {
    const float4 r0 = p.rec[4 * ((int64_t)b * p.F + f)];
    box = make_int4(__float_as_int(r0.x), __float_as_int(r0.y), __float_as_int(r0.z), __float_as_int(r0.w));
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    box.x = min(box.x, __shfl_xor(box.x, s));
    box.y = max(box.y, __shfl_xor(box.y, s));
    box.z = min(box.z, __shfl_xor(box.z, s));
    box.w = max(box.w, __shfl_xor(box.w, s));
  }
  if (lane == 0) s_box[wave] = box;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kChunk / tp::kWave; ++w) {
      const int4 o = s_box[w];
      box.x = min(box.x, o.x); box.y = max(box.y, o.y); box.z = min(box.z, o.z); box.w = max(box.w, o.w);
    }
    cbox[(int64_t)b * n_chunks + blockIdx.x] = box;
  }
}

// raster_kernel with the chunks culled first: rounds of 256 chunk boxes are tested against the tile (the four inclusive comparisons
// of the face test), the survivors' indices are compacted in ascending order into s_list, and each runs raster_chunk.  A chunk whose
// union box misses the tile holds no face whose box overlaps it, so the key minimum is taken over the same faces as in raster_kernel.
// n_chunks, the rounds and the survivor count are workgroup-uniform: every barrier is reached by all 256 threads.
__global__ void __launch_bounds__(kChunk) raster_culled_kernel(RasterParams p, int tiles_x, const int4* cbox, int n_chunks) {
  __shared__ float4 s_rec[kChunk][4];
  __shared__ int s_wave_count[kChunk / tp::kWave];
  __shared__ int s_list[kChunk];
  __shared__ int s_list_count[kChunk / tp::kWave];
  const TileCtx t = tile_ctx(p, tiles_x);
  const float4* rec = p.rec + 4 * (int64_t)t.b * p.F;
  const int4* boxes = cbox + (int64_t)t.b * n_chunks;
  unsigned long long best = ~0ull;
  for (int cbase = 0; cbase < n_chunks; cbase += kChunk) {
    const int c = cbase + t.tid;
    bool keep = false;
    if (c < n_chunks) {
      const int4 bx = boxes[c];
      keep = bx.x <= t.tx1 && bx.y >= t.tx0 && bx.z <= t.ty1 && bx.w >= t.ty0;
    }
    const unsigned long long m = __ballot(keep);
    if (t.lane == 0) s_list_count[t.wave] = __popcll(m);
    __syncthreads();
    int off = 0, n = 0;
#pragma unroll
    for (int w = 0; w < kChunk / tp::kWave; ++w) {
      const int cnt = s_list_count[w];
      off += (w < t.wave) ? cnt : 0;
      n += cnt;
    }
    if (keep) s_list[off + __popcll(m & ((1ull << t.lane) - 1ull))] = c;
    __syncthreads();
    float4 next = n > 0 ? chunk_word0(p, t, rec, s_list[0] * kChunk) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < n; ++k) {
      const float4 r0 = next;
      if (k + 1 < n) next = chunk_word0(p, t, rec, s_list[k + 1] * kChunk);          // in flight while chunk k is processed
      raster_chunk(p, t, rec, s_list[k] * kChunk, r0, s_rec, s_wave_count, best);
    }
    __syncthreads();          // (n = 0: s_list_count is rewritten next round only after every thread has read it)
  }
  raster_epilogue(p, t, rec, best);
}

// ---- 3. normals from depth ------------------------------------------------------------------------------------------------------
// compute_surfelinfo.normal_from_depth: points = centre + ray * depth with ray = R^T K^-1 (u, v, 1) (camera z component 1, not
// normalised) and centre = -R^T t; background neighbours enter with their depth of -1, unmasked; tu = p[i, j+1] - p[i, j-1],
// tv = p[i+1, j] - p[i-1, j], n = normalize(tu x tv) (eps 1e-12), third component negated; border rows / columns and pixels with
// depth <= 0 are zero.  The centre cancels in tu / tv, so they are formed from the camera-frame points K^-1 (u, v, 1) * depth and
// rotated afterwards; fp64 throughout, so the result is the exact arithmetic of the fp32 inputs to ~1e-15, not the rounding noise
// of a world-frame difference of ~700 mm points.
__device__ __forceinline__ void inv3(const float* K, double (&o)[9]) {
  const double a = K[0], b = K[1], c = K[2], d = K[3], e = K[4], f = K[5], g = K[6], h = K[7], k = K[8];
  const double A = e * k - f * h, Bc = -(d * k - f * g), C = d * h - e * g;
  const double r = 1.0 / (a * A + b * Bc + c * C);
  o[0] = A * r;  o[1] = -(b * k - c * h) * r; o[2] = (b * f - c * e) * r;
  o[3] = Bc * r; o[4] = (a * k - c * g) * r;  o[5] = -(a * f - c * d) * r;
  o[6] = C * r;  o[7] = -(a * h - b * g) * r; o[8] = (a * e - b * d) * r;
}

__global__ void __launch_bounds__(256) normal_kernel(RasterParams p) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t hw = (int64_t)p.H * p.W;
  if (gid >= (int64_t)p.B * hw) return;
  const int b = (int)(gid / hw);
  const int64_t rem = gid - (int64_t)b * hw;
  const int i = (int)(rem / p.W), j = (int)(rem - (int64_t)i * p.W);
  double n[3] = {0.0, 0.0, 0.0};
  const float* zb = p.zbuf + (int64_t)b * hw;
  if (i > 0 && j > 0 && i < p.H - 1 && j < p.W - 1 && zb[rem] > 0.0f) {
    double ki[9];
    inv3(p.intr + 9 * b, ki);
    double q[4][3];                      // camera-frame points left, right, up, down
    const int nb[4][2] = {{i, j - 1}, {i, j + 1}, {i - 1, j}, {i + 1, j}};
    for (int s = 0; s < 4; ++s) {
      const double u = nb[s][1] + 0.5, v = nb[s][0] + 0.5, d = zb[(int64_t)nb[s][0] * p.W + nb[s][1]];
      for (int r = 0; r < 3; ++r) q[s][r] = (ki[3 * r] * u + ki[3 * r + 1] * v + ki[3 * r + 2]) * d;
    }
    const float* P = p.pose + 12 * b;
    double tu[3], tv[3];
    for (int c = 0; c < 3; ++c) {       // world frame: R^T (camera-frame difference)
      tu[c] = (double)P[c] * (q[1][0] - q[0][0]) + (double)P[4 + c] * (q[1][1] - q[0][1]) + (double)P[8 + c] * (q[1][2] - q[0][2]);
      tv[c] = (double)P[c] * (q[3][0] - q[2][0]) + (double)P[4 + c] * (q[3][1] - q[2][1]) + (double)P[8 + c] * (q[3][2] - q[2][2]);
    }
    n[0] = tu[1] * tv[2] - tu[2] * tv[1];
    n[1] = tu[2] * tv[0] - tu[0] * tv[2];
    n[2] = tu[0] * tv[1] - tu[1] * tv[0];
    const double len = fmax(sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), 1e-12);
    n[0] /= len; n[1] /= len; n[2] = -n[2] / len;
  }
  for (int c = 0; c < 3; ++c) p.normal[3 * gid + c] = (float)n[c];
}

}  // namespace

extern "C" size_t tp_mesh_raster_workspace_bytes(int B, int H, int W, int F) {
  (void)H; (void)W;
  if (B <= 0 || F <= 0) return 0;
  return (size_t)B * (size_t)F * kRecFloats * sizeof(float);
}

// the face records as above, then one int4 per (image, chunk of 256 records); 64 B F is a multiple of 16, so the boxes are aligned
extern "C" size_t tp_mesh_raster_culled_workspace_bytes(int B, int H, int W, int F) {
  const size_t records = tp_mesh_raster_workspace_bytes(B, H, W, F);
  if (records == 0) return 0;
  return records + (size_t)B * (size_t)((F + kChunk - 1) / kChunk) * sizeof(int4);
}

namespace {

// both entry points: one set of checks (the messages carry the caller's name), then three launches or, culled, four
int mesh_raster_launch(const char* what, const tp_mesh_raster_args* a, tp_stream_t stream, bool culled) {
#define RASTER_REQUIRE(cond, msg)          \
  do {                                     \
    if (!(cond)) {                         \
      tp::set_error("%s: %s", what, msg);  \
      return -1;                           \
    }                                      \
  } while (0)
  RASTER_REQUIRE(a, "null pointer");
  RASTER_REQUIRE(a->B > 0 && a->B <= 65535 && a->H > 0 && a->W > 0 && a->H <= 16384 && a->W <= 16384, "bad sizes");
  RASTER_REQUIRE(a->pose && a->intr && a->zbuf, "null pointer");
  if (a->normals_from_zbuf) {
    RASTER_REQUIRE(a->normal, "normals_from_zbuf without a normal output");
    RasterParams p = {};
    p.pose = a->pose; p.intr = a->intr; p.B = a->B; p.H = a->H; p.W = a->W; p.zbuf = a->zbuf; p.normal = a->normal;
    const int64_t np = (int64_t)a->B * a->H * a->W;
    hipLaunchKernelGGL(normal_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return tp::check_launch(what);
  }
  RASTER_REQUIRE(a->V > 0 && a->F > 0, "bad sizes");
  RASTER_REQUIRE(a->verts && a->faces && a->workspace, "null pointer");
  RASTER_REQUIRE(a->rgb == nullptr || a->vcolor != nullptr, "rgb requested without vertex colours");
  RASTER_REQUIRE(a->nocs == nullptr || (a->nocs_scale[0] > 0.f && a->nocs_scale[1] > 0.f && a->nocs_scale[2] > 0.f),
                 "nocs requested with a non-positive normalisation scale");
  RASTER_REQUIRE(((uintptr_t)a->workspace & 15) == 0, "workspace must be 16-byte aligned");
#undef RASTER_REQUIRE
  RasterParams p;
  p.verts = a->verts; p.faces = a->faces; p.vcolor = a->vcolor;
  for (int c = 0; c < 3; ++c) { p.nocs_center[c] = a->nocs_center[c]; p.nocs_scale[c] = a->nocs_scale[c]; }
  p.pose = a->pose; p.intr = a->intr;
  p.B = a->B; p.H = a->H; p.W = a->W; p.V = a->V; p.F = a->F;
  p.zbuf = a->zbuf; p.face = a->face; p.rgb = a->rgb; p.nocs = a->nocs; p.normal = a->normal;
  p.rec = (float4*)a->workspace;
  hipStream_t s = (hipStream_t)stream;
  const int64_t nf = (int64_t)a->B * a->F;
  hipLaunchKernelGGL(face_setup_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, p);
  const int tiles_x = (a->W + kTile - 1) / kTile, tiles_y = (a->H + kTile - 1) / kTile;
  if (culled) {
    const int n_chunks = (a->F + kChunk - 1) / kChunk;
    int4* cbox = (int4*)(p.rec + 4 * nf);
    hipLaunchKernelGGL(chunk_box_kernel, dim3((unsigned)n_chunks, (unsigned)a->B), dim3(kChunk), 0, s, p, cbox, n_chunks);
    hipLaunchKernelGGL(raster_culled_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)a->B), dim3(kChunk), 0, s, p, tiles_x,
                       (const int4*)cbox, n_chunks);
  } else {
    hipLaunchKernelGGL(raster_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)a->B), dim3(kChunk), 0, s, p, tiles_x);
  }
  if (a->normal) {
    const int64_t np = (int64_t)a->B * a->H * a->W;
    hipLaunchKernelGGL(normal_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, p);
  }
  return tp::check_launch(what);
}

}  // namespace

extern "C" int tp_mesh_raster(const tp_mesh_raster_args* a, tp_stream_t stream) {
  return mesh_raster_launch("tp_mesh_raster", a, stream, false);
}

extern "C" int tp_mesh_raster_culled(const tp_mesh_raster_args* a, tp_stream_t stream) {
  return mesh_raster_launch("tp_mesh_raster_culled", a, stream, true);
}
