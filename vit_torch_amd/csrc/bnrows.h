// Batch statistics and per-channel sums over the rows of a token-major [M, C] tensor (C contiguous): what lpi.hip and
// convstem.hip share.  One decomposition for every size: a thread owns 16 bytes of channels (VEC = 8 bf16 or 4 fp32) of
// one row and walks rows; a workgroup of 256 threads is gt channel groups (a power of two, at most 16: 256 B of one row)
// by 256 / gt row lanes and owns (a chunk of consecutive rows) x (a tile of gt * VEC channels).
//
// Statistics: each thread runs Welford's update over its rows (fp32), the workgroup combines its lanes with Chan's formula
// in lane order, stat_kernel combines the chunks in chunk order (both combinations in double, the counts analytic): no raw
// E[u^2] - E[u]^2, no atomics, bitwise repeatable.  A constant channel gives M2 = 0 exactly.  All other sums are
// per-thread, then per-workgroup in lane order (lane_sum_store), then vitmi_reduce_rows' fixed order.
//
// Included inside the including file's anonymous namespace.
#pragma once

constexpr int NT = 256;
constexpr int MAX_GT = 16;          // channel groups of a workgroup: 16 x 16 B = 256 B of a token row
constexpr int MAX_TC = MAX_GT * 8;  // channels of a tile, at most
constexpr int TARGET_WG = 1024;     // workgroups per pass, about: four per CU

struct Geo {
  int vec, G, gt, gt_log2, tiles, PL, chunk, nch;
  int64_t M;
};

inline Geo row_geometry(int dtype, int64_t M, int64_t C) {
  Geo g;
  g.vec = dtype == VITMI_BF16 ? 8 : 4;
  g.G = (int)(C / g.vec);
  g.gt = 1;
  g.gt_log2 = 0;
  while (g.gt < MAX_GT && g.gt < g.G) { g.gt *= 2; ++g.gt_log2; }
  g.tiles = (g.G + g.gt - 1) / g.gt;
  g.PL = NT / g.gt;
  g.M = M;
  const int64_t target = TARGET_WG / g.tiles > 0 ? TARGET_WG / g.tiles : 1;
  int64_t per = (g.M + target - 1) / target;
  if (per < 4 * g.PL) per = 4 * g.PL;
  g.chunk = (int)((per + g.PL - 1) / g.PL * g.PL);
  g.nch = (int)((g.M + g.chunk - 1) / g.chunk);
  return g;
}

struct RowDims { int C, chunk, gt_log2; int64_t M; };

inline size_t round256(size_t n) { return (n + 255) / 256 * 256; }

// ---- 16-byte channel vectors as fp32 ----
template <typename T> struct Vec;
template <> struct Vec<bf16> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void load(const bf16* p, float* v) {
    const bf16x8 r = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)r[e];
  }
  // stores v rounded to bf16 and leaves the rounded values in v
  static __device__ __forceinline__ void store(bf16* p, float* v) {
    bf16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) { r[e] = (bf16)v[e]; v[e] = (float)r[e]; }
    *reinterpret_cast<bf16x8*>(p) = r;
  }
};
template <> struct Vec<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const f32x4 r = *reinterpret_cast<const f32x4*>(p);
    v[0] = r[0]; v[1] = r[1]; v[2] = r[2]; v[3] = r[3];
  }
  static __device__ __forceinline__ void store(float* p, float* v) {
    const f32x4 r = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p) = r;
  }
};

template <int V> __device__ __forceinline__ void loadf(const float* p, float* v) {
#pragma unroll
  for (int e = 0; e < V; e += 4) {
    const f32x4 r = *reinterpret_cast<const f32x4*>(p + e);
    v[e] = r[0]; v[e + 1] = r[1]; v[e + 2] = r[2]; v[e + 3] = r[3];
  }
}

// a workgroup's place: its channel group, its row lane, its rows.  D: RowDims or a struct that extends it.
struct Place {
  int gl, pl, gt, PL, TC, c_base, c0;
  bool active;
  int64_t p_begin, p_end;
  template <int V, typename D> __device__ __forceinline__ void init(const D& d) {
    gt = 1 << d.gt_log2;
    PL = NT >> d.gt_log2;
    gl = threadIdx.x & (gt - 1);
    pl = threadIdx.x >> d.gt_log2;
    TC = gt * V;
    c_base = blockIdx.y * TC;
    c0 = c_base + gl * V;
    active = c0 < d.C;
    p_begin = (int64_t)blockIdx.x * d.chunk;
    p_end = p_begin + d.chunk < d.M ? p_begin + d.chunk : d.M;
  }
};

// sum of a[v] over the row lanes of each channel group, in lane order, to dst[(channel of the tile) * stride]
template <int V>
__device__ __forceinline__ void lane_sum_store(float* red, const float* a, const Place& pc, float* dst, int stride, int C) {
#pragma unroll
  for (int v = 0; v < V; ++v) red[threadIdx.x * V + v] = a[v];
  __syncthreads();
  if (threadIdx.x < pc.TC) {
    const int g = threadIdx.x / V, v = threadIdx.x - g * V;
    float s = 0.f;
    for (int l = 0; l < pc.PL; ++l) s += red[(l * pc.gt + g) * V + v];
    if (pc.c_base + threadIdx.x < C) dst[(int64_t)threadIdx.x * stride] = s;
  }
  __syncthreads();
}

// one more value per channel into a thread's running (count n, mean, M2): n is the count INCLUDING this value
template <int V>
__device__ __forceinline__ void welford_step(const float* x, float n, float* mean, float* m2) {
  const float inv = 1.f / n;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const float dl = x[v] - mean[v];
    mean[v] += dl * inv;
    m2[v] = fmaf(dl, x[v] - mean[v], m2[v]);
  }
}

// the lanes' (n, mean, M2) in lane order -> the workgroup's (mean, M2) of its chunk to part[chunk][2][C] (double);
// red: 2 * NT * V floats, cnt: NT floats
template <int V>
__device__ __forceinline__ void welford_block_store(float* red, float* cnt, const float* mean, const float* m2, float n,
                                                    const Place& pc, double* part, int C) {
#pragma unroll
  for (int v = 0; v < V; ++v) { red[threadIdx.x * V + v] = mean[v]; red[(NT + threadIdx.x) * V + v] = m2[v]; }
  cnt[threadIdx.x] = n;
  __syncthreads();
  if (threadIdx.x < pc.TC && pc.c_base + threadIdx.x < C) {
    const int g = threadIdx.x / V, v = threadIdx.x - g * V;
    double na = 0., ma = 0., sa = 0.;            // the combination in double: it costs nothing here
    for (int l = 0; l < pc.PL; ++l) {
      const int t = l * pc.gt + g;
      const double nb = cnt[t];
      if (nb > 0.) {
        const double mb = red[t * V + v], sb = red[(NT + t) * V + v], nn = na + nb, dl = mb - ma;
        ma += dl * (nb / nn);
        sa += sb + dl * dl * (na * nb / nn);
        na = nn;
      }
    }
    double* row = part + (int64_t)blockIdx.x * 2 * C + pc.c_base + threadIdx.x;
    row[0] = ma;
    row[C] = sa;
  }
}

// the chunks' (count, mean, M2) in chunk order -> stat = (mean, rstd); the running buffers in place
__global__ __launch_bounds__(NT) void stat_kernel(const double* __restrict__ part, int nch, RowDims d, float momentum, float eps,
                                                  float* __restrict__ stat, float* __restrict__ rmean,
                                                  float* __restrict__ rvar, int64_t* __restrict__ nbt) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c == 0 && nbt) nbt[0] += 1;
  if (c >= d.C) return;
  double na = 0., ma = 0., sa = 0.;
  for (int k = 0; k < nch; ++k) {
    const int64_t left = d.M - (int64_t)k * d.chunk;
    const double nb = (double)(left < d.chunk ? left : d.chunk);
    const double mb = part[(int64_t)k * 2 * d.C + c], sb = part[(int64_t)k * 2 * d.C + d.C + c], nn = na + nb, dl = mb - ma;
    ma += dl * (nb / nn);
    sa += sb + dl * dl * (na * nb / nn);
    na = nn;
  }
  const double m = momentum;
  stat[c] = (float)ma;
  stat[d.C + c] = (float)(1. / sqrt(sa / (double)d.M + (double)eps));
  if (rmean) rmean[c] = (float)((1. - m) * rmean[c] + m * ma);
  if (rvar) rvar[c] = (float)((1. - m) * rvar[c] + m * (sa / (double)(d.M - 1)));
}

__global__ __launch_bounds__(NT) void eval_stat_kernel(const float* __restrict__ rmean, const float* __restrict__ rvar, int C,
                                                       float eps, float* __restrict__ stat) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= C) return;
  stat[c] = rmean[c];
  stat[C + c] = 1.f / sqrtf(rvar[c] + eps);
}

// per-thread batch-norm constants of its channels
template <int V> struct Norm {
  float mean[V], rstd[V], gamma[V], beta[V];
  __device__ __forceinline__ void load(const float* stat, const float* g, const float* b, int C, int c0) {
    loadf<V>(stat + c0, mean);
    loadf<V>(stat + C + c0, rstd);
    loadf<V>(g + c0, gamma);
    loadf<V>(b + c0, beta);
  }
};
