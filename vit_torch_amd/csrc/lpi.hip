// XCiT's local patch interaction (LPI, models/xcit.py:111-141 of the reference) on token-major rows: x [B, H*W, C] with C
// contiguous, exactly as layernorm_fwd leaves it.  No NCHW copy exists anywhere.  Per channel, with w1, w2 the depthwise
// 3 x 3 taps (cross-correlation, zero padding), M = B*H*W:
//   c = conv1(x) + b1        u = gelu(c), STORED in the compute dtype        mean, var = batch statistics of u AS STORED
//   uh = (u - mean) rstd     z = uh gamma + beta      out = conv2(z) + b2    (the padding of conv2 is of z: a border tap adds 0)
// and, for dout:
//   dz = conv2^T(dout)       dbeta = sum dz     dgamma = sum dz uh     db2 = sum dout     dw2[t] = sum_q z[q] dout[q - t]
//   du = gamma rstd (dz - dbeta/M - uh dgamma/M)      (eval: du = gamma rstd dz, rstd from running_var)
//   dc = du gelu'(c), c recomputed from x             db1 = sum dc     dw1[t] = sum_p dc[p] x[p + t]       dx = conv1^T(dc)
//
// Shape of the work.  Every kernel uses ONE decomposition, for every grid size (there is no resident / banded switch): a
// thread owns 16 bytes of channels (VEC = 8 bf16 or 4 fp32) of one position and walks positions; a workgroup of 256
// threads is gt channel groups (a power of two, at most 16: 256 B of one token row) by 256 / gt position lanes and owns
// (a chunk of consecutive positions of the flattened batch) x (a tile of gt * VEC channels).  The eight neighbours of a
// position are read from global memory with the same 16-byte accesses: they are rows the neighbouring lanes and the
// previous / next grid row of the same workgroup also read, so they come from L1 / L2 and each tensor crosses HBM once per
// pass.  The taps of the tile are staged in LDS as [tap][channel] (two 16-byte reads per tap).  Nothing else is in LDS but
// the reduction scratch: 9 KB of taps + 16 KB.
//
// The two-deep halo of the backward (dx needs dc on a ring, dc needs dz and c on that ring, those need dout and x on the
// next ring) is cut by ONE staged tensor: dc, in the compute dtype, in the workspace.  In bf16 that is a declared rounding
// (dx sees dc rounded to bf16; db1 and dw1 are summed from the unrounded fp32 dc).
//
// Passes (T = bytes of one [B, N, C] tensor):
//   forward, training   conv1_kernel: x -> u, per-workgroup (mean, M2) partials            reads x, writes u         2T
//                       stat_kernel:  Chan's combination of the partials in chunk order -> stat [2, C] = (mean, rstd),
//                                     running_mean / running_var / num_batches_tracked updated in place   (C-sized)
//                       conv2_kernel: u -> out                                               reads u, writes out       2T
//   forward, eval       conv1_kernel (no statistics), eval_stat_kernel: stat = (running_mean, 1/sqrt(running_var + eps)),
//                       conv2_kernel; no buffer is touched
//   backward            red_kernel:   dout, u -> partials of dbeta | dgamma | db2 | dw2      reads dout, u             2T
//                       vitmi_reduce_rows_segs: the four gradients
//                       dc_kernel:    dout, u, x -> dc; partials of db1 | dw1                reads 3, writes dc         4T
//                       vitmi_reduce_rows x 2
//                       dx_kernel:    dc -> dx                                               reads dc, writes dx        2T
// Forward 4T, backward 8T: the 6T of a halo-in-LDS form plus the write and the read of the one staged tensor.
//
// Statistics: each thread runs Welford's update over its positions, the workgroup combines its lanes with Chan's formula in
// lane order, stat_kernel combines the chunks in chunk order (both combinations in double): no raw E[u^2] - E[u]^2, no atomics, bitwise repeatable.  A
// constant channel gives M2 = 0 exactly.  All other sums are per-thread, then per-workgroup in lane order, then
// vitmi_reduce_rows' fixed order.
#include "common.h"

namespace {

#include "bnrows.h"     // the row decomposition, Vec, Place, the Welford / Chan statistics and stat_kernel (shared with convstem.hip)

Geo geometry(int dtype, int64_t B, int64_t H, int64_t W, int64_t C) { return row_geometry(dtype, B * H * W, C); }

struct Dims : RowDims { int H, W; };

// the tile's taps as [tap][channel of the tile] (zero past C)
__device__ __forceinline__ void stage_taps(float* sw, const float* __restrict__ w, int c_base, int TC, int C) {
  for (int i = threadIdx.x; i < 9 * TC; i += NT) {
    const int t = i / TC, cc = i - t * TC, c = c_base + cc;
    sw[i] = c < C ? w[(int64_t)c * 9 + t] : 0.f;
  }
}

// -------------------------------------------------------------------------------------------------- forward ---
// u = gelu(conv1(x) + b1), stored; with STATS the workgroup's (mean, M2) of the stored values to part[chunk][2][C] (double)
template <typename T, bool STATS>
__global__ __launch_bounds__(NT) void conv1_kernel(const T* __restrict__ x, const float* __restrict__ w1,
                                                   const float* __restrict__ b1, T* __restrict__ u,
                                                   double* __restrict__ part, Dims d) {
  constexpr int V = Vec<T>::N;
  __shared__ __attribute__((aligned(16))) float sw[9 * MAX_TC];
  __shared__ __attribute__((aligned(16))) float red[STATS ? 2 * NT * V : 4];
  __shared__ float cnt[STATS ? NT : 1];
  Place pc;
  pc.init<V>(d);
  stage_taps(sw, w1, pc.c_base, pc.TC, d.C);
  __syncthreads();
  float bias[V], mean[V], m2[V];
#pragma unroll
  for (int v = 0; v < V; ++v) { bias[v] = 0.f; mean[v] = 0.f; m2[v] = 0.f; }
  if (pc.active) loadf<V>(b1 + pc.c0, bias);
  float n = 0.f;
  const int HW = d.H * d.W;
  if (pc.active) {
    for (int64_t p = pc.p_begin + pc.pl; p < pc.p_end; p += pc.PL) {
      const int r = (int)p % HW, h = r / d.W, w = r - h * d.W;
      float acc[V];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = bias[v];
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          if ((unsigned)(h + dy) < (unsigned)d.H && (unsigned)(w + dx) < (unsigned)d.W) {
            float xv[V], wv[V];
            Vec<T>::load(x + (p + dy * d.W + dx) * d.C + pc.c0, xv);
            loadf<V>(sw + ((dy + 1) * 3 + dx + 1) * pc.TC + pc.gl * V, wv);
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = fmaf(wv[v], xv[v], acc[v]);
          }
        }
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = gelu_erf(acc[v]);
      Vec<T>::store(u + p * d.C + pc.c0, acc);         // acc now holds the values as stored
      if (STATS) {
        n += 1.f;
        welford_step<V>(acc, n, mean, m2);
      }
    }
  }
  if (STATS) welford_block_store<V>(red, cnt, mean, m2, n, pc, part, d.C);
}

// out = conv2(z) + b2, z = (u - mean) rstd gamma + beta inside the grid and 0 outside
template <typename T>
__global__ __launch_bounds__(NT) void conv2_kernel(const T* __restrict__ u, const float* __restrict__ stat,
                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   const float* __restrict__ w2, const float* __restrict__ b2,
                                                   T* __restrict__ out, Dims d) {
  constexpr int V = Vec<T>::N;
  __shared__ __attribute__((aligned(16))) float sw[9 * MAX_TC];
  Place pc;
  pc.init<V>(d);
  stage_taps(sw, w2, pc.c_base, pc.TC, d.C);
  __syncthreads();
  if (!pc.active) return;
  Norm<V> nm;
  nm.load(stat, gamma, beta, d.C, pc.c0);
  float bias[V];
  loadf<V>(b2 + pc.c0, bias);
  const int HW = d.H * d.W;
  for (int64_t p = pc.p_begin + pc.pl; p < pc.p_end; p += pc.PL) {
    const int r = (int)p % HW, h = r / d.W, w = r - h * d.W;
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = bias[v];
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if ((unsigned)(h + dy) < (unsigned)d.H && (unsigned)(w + dx) < (unsigned)d.W) {
          float uv[V], wv[V];
          Vec<T>::load(u + (p + dy * d.W + dx) * d.C + pc.c0, uv);
          loadf<V>(sw + ((dy + 1) * 3 + dx + 1) * pc.TC + pc.gl * V, wv);
#pragma unroll
          for (int v = 0; v < V; ++v) {
            const float z = fmaf((uv[v] - nm.mean[v]) * nm.rstd[v], nm.gamma[v], nm.beta[v]);
            acc[v] = fmaf(wv[v], z, acc[v]);
          }
        }
      }
    Vec<T>::store(out + p * d.C + pc.c0, acc);
  }
}

// ------------------------------------------------------------------------------------------------- backward ---
// partial row of the chunk: dbeta [C] | dgamma [C] | db2 [C] | dw2 [C][9]
template <typename T>
__global__ __launch_bounds__(NT) void red_kernel(const T* __restrict__ dout, const T* __restrict__ u,
                                                 const float* __restrict__ stat, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, const float* __restrict__ w2,
                                                 float* __restrict__ part, Dims d) {
  constexpr int V = Vec<T>::N;
  __shared__ __attribute__((aligned(16))) float sw[9 * MAX_TC];
  __shared__ __attribute__((aligned(16))) float red[NT * V];
  Place pc;
  pc.init<V>(d);
  stage_taps(sw, w2, pc.c_base, pc.TC, d.C);
  __syncthreads();
  float dbeta[V], dgamma[V], db2[V], dw2[9][V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    dbeta[v] = dgamma[v] = db2[v] = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) dw2[t][v] = 0.f;
  }
  if (pc.active) {
    Norm<V> nm;
    nm.load(stat, gamma, beta, d.C, pc.c0);
    const int HW = d.H * d.W;
    for (int64_t p = pc.p_begin + pc.pl; p < pc.p_end; p += pc.PL) {
      const int r = (int)p % HW, h = r / d.W, w = r - h * d.W;
      float uh[V], z[V], dz[V];
      Vec<T>::load(u + p * d.C + pc.c0, uh);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        uh[v] = (uh[v] - nm.mean[v]) * nm.rstd[v];
        z[v] = fmaf(uh[v], nm.gamma[v], nm.beta[v]);
        dz[v] = 0.f;
      }
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          if ((unsigned)(h + dy) < (unsigned)d.H && (unsigned)(w + dx) < (unsigned)d.W) {
            const int t = (1 - dy) * 3 + (1 - dx);       // out[p + o] reads z[p] through tap -o
            float dv[V], wv[V];
            Vec<T>::load(dout + (p + dy * d.W + dx) * d.C + pc.c0, dv);
            loadf<V>(sw + t * pc.TC + pc.gl * V, wv);
#pragma unroll
            for (int v = 0; v < V; ++v) {
              dz[v] = fmaf(wv[v], dv[v], dz[v]);
              dw2[t][v] = fmaf(dv[v], z[v], dw2[t][v]);
              if (dy == 0 && dx == 0) db2[v] += dv[v];
            }
          }
        }
#pragma unroll
      for (int v = 0; v < V; ++v) {
        dbeta[v] += dz[v];
        dgamma[v] = fmaf(dz[v], uh[v], dgamma[v]);
      }
    }
  }
  float* row = part + (int64_t)blockIdx.x * 12 * d.C;
  lane_sum_store<V>(red, dbeta, pc, row + pc.c_base, 1, d.C);
  lane_sum_store<V>(red, dgamma, pc, row + d.C + pc.c_base, 1, d.C);
  lane_sum_store<V>(red, db2, pc, row + 2 * d.C + pc.c_base, 1, d.C);
#pragma unroll
  for (int t = 0; t < 9; ++t) lane_sum_store<V>(red, dw2[t], pc, row + 3 * d.C + (int64_t)pc.c_base * 9 + t, 9, d.C);
}

// dc = du gelu'(c) staged in the compute dtype; partial row of the chunk: db1 [C] | dw1 [C][9] from the unrounded dc
template <typename T, bool TRAIN>
__global__ __launch_bounds__(NT) void dc_kernel(const T* __restrict__ x, const T* __restrict__ u, const T* __restrict__ dout,
                                                const float* __restrict__ stat, const float* __restrict__ gamma,
                                                const float* __restrict__ w1, const float* __restrict__ b1,
                                                const float* __restrict__ w2, const float* __restrict__ dgamma,
                                                const float* __restrict__ dbeta, T* __restrict__ dc,
                                                float* __restrict__ part, Dims d) {
  constexpr int V = Vec<T>::N;
  __shared__ __attribute__((aligned(16))) float sw1[9 * MAX_TC];
  __shared__ __attribute__((aligned(16))) float sw2[9 * MAX_TC];
  __shared__ __attribute__((aligned(16))) float red[NT * V];
  Place pc;
  pc.init<V>(d);
  stage_taps(sw1, w1, pc.c_base, pc.TC, d.C);
  stage_taps(sw2, w2, pc.c_base, pc.TC, d.C);
  __syncthreads();
  float db1[V], dw1[9][V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    db1[v] = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) dw1[t][v] = 0.f;
  }
  if (pc.active) {
    float mean[V], rstd[V], gr[V], mdz[V], mdzu[V], bias[V];
    loadf<V>(stat + pc.c0, mean);
    loadf<V>(stat + d.C + pc.c0, rstd);
    loadf<V>(gamma + pc.c0, gr);
    loadf<V>(b1 + pc.c0, bias);
    loadf<V>(dbeta + pc.c0, mdz);
    loadf<V>(dgamma + pc.c0, mdzu);
    const float invM = 1.f / (float)d.M;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      gr[v] *= rstd[v];
      mdz[v] = TRAIN ? mdz[v] * invM : 0.f;
      mdzu[v] = TRAIN ? mdzu[v] * invM : 0.f;
    }
    const int HW = d.H * d.W;
    for (int64_t p = pc.p_begin + pc.pl; p < pc.p_end; p += pc.PL) {
      const int r = (int)p % HW, h = r / d.W, w = r - h * d.W;
      float dz[V], c[V], xv[9][V];
#pragma unroll
      for (int v = 0; v < V; ++v) { dz[v] = 0.f; c[v] = bias[v]; }
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int t = (dy + 1) * 3 + dx + 1;
          if ((unsigned)(h + dy) < (unsigned)d.H && (unsigned)(w + dx) < (unsigned)d.W) {
            float dv[V], wa[V], wb[V];
            const int64_t off = (p + dy * d.W + dx) * d.C + pc.c0;
            Vec<T>::load(x + off, xv[t]);
            Vec<T>::load(dout + off, dv);
            loadf<V>(sw1 + t * pc.TC + pc.gl * V, wa);
            loadf<V>(sw2 + (8 - t) * pc.TC + pc.gl * V, wb);
#pragma unroll
            for (int v = 0; v < V; ++v) {
              c[v] = fmaf(wa[v], xv[t][v], c[v]);
              dz[v] = fmaf(wb[v], dv[v], dz[v]);
            }
          } else {
#pragma unroll
            for (int v = 0; v < V; ++v) xv[t][v] = 0.f;
          }
        }
      float uh[V], g[V];
      Vec<T>::load(u + p * d.C + pc.c0, uh);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        uh[v] = (uh[v] - mean[v]) * rstd[v];
        const float du = gr[v] * (TRAIN ? dz[v] - mdz[v] - uh[v] * mdzu[v] : dz[v]);
        g[v] = du * dgelu_erf(c[v]);
        db1[v] += g[v];
#pragma unroll
        for (int t = 0; t < 9; ++t) dw1[t][v] = fmaf(g[v], xv[t][v], dw1[t][v]);
      }
      Vec<T>::store(dc + p * d.C + pc.c0, g);
    }
  }
  float* row = part + (int64_t)blockIdx.x * 10 * d.C;
  lane_sum_store<V>(red, db1, pc, row + pc.c_base, 1, d.C);
#pragma unroll
  for (int t = 0; t < 9; ++t) lane_sum_store<V>(red, dw1[t], pc, row + d.C + (int64_t)pc.c_base * 9 + t, 9, d.C);
}

// dx = conv1^T(dc)
template <typename T>
__global__ __launch_bounds__(NT) void dx_kernel(const T* __restrict__ dc, const float* __restrict__ w1, T* __restrict__ dx,
                                                Dims d) {
  constexpr int V = Vec<T>::N;
  __shared__ __attribute__((aligned(16))) float sw[9 * MAX_TC];
  Place pc;
  pc.init<V>(d);
  stage_taps(sw, w1, pc.c_base, pc.TC, d.C);
  __syncthreads();
  if (!pc.active) return;
  const int HW = d.H * d.W;
  for (int64_t p = pc.p_begin + pc.pl; p < pc.p_end; p += pc.PL) {
    const int r = (int)p % HW, h = r / d.W, w = r - h * d.W;
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx_ = -1; dx_ <= 1; ++dx_) {
        if ((unsigned)(h + dy) < (unsigned)d.H && (unsigned)(w + dx_) < (unsigned)d.W) {
          float gv[V], wv[V];
          Vec<T>::load(dc + (p + dy * d.W + dx_) * d.C + pc.c0, gv);
          loadf<V>(sw + ((1 - dy) * 3 + (1 - dx_)) * pc.TC + pc.gl * V, wv);
#pragma unroll
          for (int v = 0; v < V; ++v) acc[v] = fmaf(wv[v], gv[v], acc[v]);
        }
      }
    Vec<T>::store(dx + p * d.C + pc.c0, acc);
  }
}

// ---------------------------------------------------------------------------------------------------- dispatch ---
size_t dc_bytes(int dtype, const Geo& g, int64_t C) { return round256((size_t)g.M * (size_t)C * dtype_size(dtype)); }

int check_shape(const char* who, int dtype, int64_t B, int64_t H, int64_t W, int64_t C, int training) {
  VITMI_REQUIRE(dtype == VITMI_BF16 || dtype == VITMI_F32, VITMI_E_DTYPE, "%s: activations must be bf16 or fp32", who);
  VITMI_REQUIRE(C >= 8 && C % 8 == 0 && C < (1 << 20), VITMI_E_SHAPE, "%s: C = %lld must be a multiple of 8 (below 2^20)", who,
                (long long)C);
  VITMI_REQUIRE(B >= 1 && H >= 1 && W >= 1 && H < (1 << 15) && W < (1 << 15) && B < (1ll << 31) && B * H * W < (1ll << 31),
                VITMI_E_SHAPE, "%s: B = %lld, H = %lld, W = %lld: every extent must be at least 1 (B*H*W < 2^31)", who,
                (long long)B, (long long)H, (long long)W);
  VITMI_REQUIRE(!training || B * H * W > 1, VITMI_E_SHAPE,
                "%s: training needs more than one position per channel (B*H*W = 1): the batch variance is undefined", who);
  return 0;
}

Dims dims_of(const Geo& g, int64_t H, int64_t W, int64_t C) {
  Dims d;
  d.H = (int)H; d.W = (int)W; d.C = (int)C; d.chunk = g.chunk; d.gt_log2 = g.gt_log2; d.M = g.M;
  return d;
}

template <typename T>
int fwd(const T* x, const float* w1, const float* b1, const float* gamma, const float* beta, const float* w2, const float* b2,
        float* rmean, float* rvar, int64_t* nbt, T* u, float* stat, T* out, int training, float momentum, float eps,
        const Geo& g, const Dims& d, float* part, hipStream_t s) {
  const dim3 grid((unsigned)g.nch, (unsigned)g.tiles), cgrid((unsigned)((d.C + NT - 1) / NT));
  if (training) {
    hipLaunchKernelGGL((conv1_kernel<T, true>), grid, dim3(NT), 0, s, x, w1, b1, u, reinterpret_cast<double*>(part), d);
    if (int rc = vitmi_check_launch("lpi conv1_kernel")) return rc;
    hipLaunchKernelGGL(stat_kernel, cgrid, dim3(NT), 0, s, reinterpret_cast<const double*>(part), g.nch, d, momentum, eps, stat, rmean, rvar, nbt);
    if (int rc = vitmi_check_launch("lpi stat_kernel")) return rc;
  } else {
    hipLaunchKernelGGL((conv1_kernel<T, false>), grid, dim3(NT), 0, s, x, w1, b1, u, (double*)nullptr, d);
    if (int rc = vitmi_check_launch("lpi conv1_kernel")) return rc;
    hipLaunchKernelGGL(eval_stat_kernel, cgrid, dim3(NT), 0, s, (const float*)rmean, (const float*)rvar, d.C, eps, stat);
    if (int rc = vitmi_check_launch("lpi eval_stat_kernel")) return rc;
  }
  hipLaunchKernelGGL((conv2_kernel<T>), grid, dim3(NT), 0, s, (const T*)u, (const float*)stat, gamma, beta, w2, b2, out, d);
  return vitmi_check_launch("lpi conv2_kernel");
}

template <typename T>
int bwd(const T* x, const T* u, const T* dout, const float* stat, const float* w1, const float* b1, const float* gamma,
        const float* beta, const float* w2, T* dx, float* dw1, float* db1, float* dgamma, float* dbeta, float* dw2, float* db2,
        int training, const Geo& g, const Dims& d, T* dc, float* part, hipStream_t s) {
  const dim3 grid((unsigned)g.nch, (unsigned)g.tiles);
  const int C = d.C;
  hipLaunchKernelGGL((red_kernel<T>), grid, dim3(NT), 0, s, dout, u, stat, gamma, beta, w2, part, d);
  if (int rc = vitmi_check_launch("lpi red_kernel")) return rc;
  float* const outs[4] = {dbeta, dgamma, db2, dw2};
  const int width[4] = {C, C, C, 9 * C};
  if (int rc = vitmi_reduce_rows_segs(part, g.nch, 12 * (int64_t)C, outs, width, s)) return rc;
  if (training)
    hipLaunchKernelGGL((dc_kernel<T, true>), grid, dim3(NT), 0, s, x, u, dout, stat, gamma, w1, b1, w2, (const float*)dgamma,
                       (const float*)dbeta, dc, part, d);
  else
    hipLaunchKernelGGL((dc_kernel<T, false>), grid, dim3(NT), 0, s, x, u, dout, stat, gamma, w1, b1, w2, (const float*)dgamma,
                       (const float*)dbeta, dc, part, d);
  if (int rc = vitmi_check_launch("lpi dc_kernel")) return rc;
  if (int rc = vitmi_reduce_rows(part, g.nch, C, 10 * (int64_t)C, db1, s)) return rc;
  if (int rc = vitmi_reduce_rows(part + C, g.nch, 9 * (int64_t)C, 10 * (int64_t)C, dw1, s)) return rc;
  hipLaunchKernelGGL((dx_kernel<T>), grid, dim3(NT), 0, s, (const T*)dc, w1, dx, d);
  return vitmi_check_launch("lpi dx_kernel");
}

}  // namespace

extern "C" int vitmi_lpi_supported(int dtype, int64_t B, int64_t H, int64_t W, int64_t C) {
  return (dtype == VITMI_BF16 || dtype == VITMI_F32) && C >= 8 && C % 8 == 0 && C < (1 << 20) && B >= 1 && H >= 1 && W >= 1 &&
         H < (1 << 15) && W < (1 << 15) && B < (1ll << 31) && B * H * W < (1ll << 31);
}

// the staged dc [B, H*W, C] in the compute dtype, then the per-chunk partial rows (12 C floats, the widest pass)
extern "C" size_t vitmi_lpi_workspace(int dtype, int64_t B, int64_t H, int64_t W, int64_t C) {
  if (!vitmi_lpi_supported(dtype, B, H, W, C)) return 0;
  const Geo g = geometry(dtype, B, H, W, C);
  return dc_bytes(dtype, g, C) + round256((size_t)g.nch * 12 * (size_t)C * sizeof(float));
}

extern "C" int vitmi_lpi_fwd(const void* x, const float* w1, const float* b1, const float* gamma, const float* beta,
                             const float* w2, const float* b2, float* running_mean, float* running_var,
                             int64_t* num_batches_tracked, void* u, float* stat, void* out, int dtype, int training,
                             float momentum, float eps, int64_t B, int64_t H, int64_t W, int64_t C, void* workspace,
                             size_t workspace_bytes, void* stream) {
  if (int rc = check_shape("lpi_fwd", dtype, B, H, W, C, training)) return rc;
  VITMI_REQUIRE(x && w1 && b1 && gamma && beta && w2 && b2 && u && stat && out, VITMI_E_BADARG, "lpi_fwd: null pointer");
  VITMI_REQUIRE(training || (running_mean && running_var), VITMI_E_BADARG, "lpi_fwd: eval mode needs the running buffers");
  VITMI_REQUIRE(is_aligned(x, 16) && is_aligned(u, 16) && is_aligned(out, 16) && is_aligned(stat, 16) && is_aligned(w1, 16) &&
                    is_aligned(w2, 16) && is_aligned(b1, 16) && is_aligned(b2, 16) && is_aligned(gamma, 16) &&
                    is_aligned(beta, 16) && is_aligned(running_mean, 4) && is_aligned(running_var, 4) &&
                    is_aligned(num_batches_tracked, 8),
                VITMI_E_ALIGN, "lpi_fwd: x, u, out, stat and the parameters must be 16-B aligned");
  VITMI_REQUIRE(workspace && is_aligned(workspace, 16) && workspace_bytes >= vitmi_lpi_workspace(dtype, B, H, W, C),
                VITMI_E_WORKSPACE, "lpi_fwd: workspace missing, not 16-B aligned or smaller than vitmi_lpi_workspace");
  const Geo g = geometry(dtype, B, H, W, C);
  const Dims d = dims_of(g, H, W, C);
  float* part = reinterpret_cast<float*>(static_cast<char*>(workspace) + dc_bytes(dtype, g, C));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == VITMI_BF16)
    return fwd<bf16>((const bf16*)x, w1, b1, gamma, beta, w2, b2, running_mean, running_var, num_batches_tracked, (bf16*)u, stat,
                     (bf16*)out, training, momentum, eps, g, d, part, s);
  return fwd<float>((const float*)x, w1, b1, gamma, beta, w2, b2, running_mean, running_var, num_batches_tracked, (float*)u, stat,
                    (float*)out, training, momentum, eps, g, d, part, s);
}

extern "C" int vitmi_lpi_bwd(const void* x, const void* u, const void* dout, const float* stat, const float* w1,
                             const float* b1, const float* gamma, const float* beta, const float* w2, void* dx, float* dw1,
                             float* db1, float* dgamma, float* dbeta, float* dw2, float* db2, int dtype, int training,
                             int64_t B, int64_t H, int64_t W, int64_t C, void* workspace, size_t workspace_bytes,
                             void* stream) {
  if (int rc = check_shape("lpi_bwd", dtype, B, H, W, C, training)) return rc;
  VITMI_REQUIRE(x && u && dout && stat && w1 && b1 && gamma && beta && w2 && dx && dw1 && db1 && dgamma && dbeta && dw2 && db2,
                VITMI_E_BADARG, "lpi_bwd: null pointer");
  VITMI_REQUIRE(is_aligned(x, 16) && is_aligned(u, 16) && is_aligned(dout, 16) && is_aligned(dx, 16) && is_aligned(stat, 16) &&
                    is_aligned(w1, 16) && is_aligned(w2, 16) && is_aligned(b1, 16) && is_aligned(gamma, 16) &&
                    is_aligned(beta, 16) && is_aligned(dw1, 4) && is_aligned(db1, 4) && is_aligned(dgamma, 16) &&
                    is_aligned(dbeta, 16) && is_aligned(dw2, 4) && is_aligned(db2, 4),
                VITMI_E_ALIGN, "lpi_bwd: x, u, dout, dx, stat, the parameters, dgamma and dbeta must be 16-B aligned");
  VITMI_REQUIRE(workspace && is_aligned(workspace, 16) && workspace_bytes >= vitmi_lpi_workspace(dtype, B, H, W, C),
                VITMI_E_WORKSPACE, "lpi_bwd: workspace missing, not 16-B aligned or smaller than vitmi_lpi_workspace");
  const Geo g = geometry(dtype, B, H, W, C);
  const Dims d = dims_of(g, H, W, C);
  float* part = reinterpret_cast<float*>(static_cast<char*>(workspace) + dc_bytes(dtype, g, C));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == VITMI_BF16)
    return bwd<bf16>((const bf16*)x, (const bf16*)u, (const bf16*)dout, stat, w1, b1, gamma, beta, w2, (bf16*)dx, dw1, db1, dgamma,
                     dbeta, dw2, db2, training, g, d, (bf16*)workspace, part, s);
  return bwd<float>((const float*)x, (const float*)u, (const float*)dout, stat, w1, b1, gamma, beta, w2, (float*)dx, dw1, db1,
                    dgamma, dbeta, dw2, db2, training, g, d, (float*)workspace, part, s);
}
