// XCiT's Fourier positional encoding and the element-wise glue of its class-attention block (models/xcit.py:20-55 and
// :176-218 of the reference).  Every kernel here is bandwidth-bound: a thread moves one 16-byte vector of the fp32 stream
// (four channels; the operand-dtype tensors beside it as 8- or 16-byte vectors), grids are sized by the data and capped
// where a kernel strides, no atomics, fp32 arithmetic throughout.
//
//   vitmi_posfourier_features   out [Hp*Wp, 2*hidden] (bf16 or fp32), hidden = 32: for the pixel (y, x) the hidden y-features
//                               then the hidden x-features; feature j of a coordinate i on an axis of n pixels is
//                               t = ((i + 1) / (n + 1e-6) * 2 pi) / temperature^(2 (j / 2) / hidden), sin(t) for even j and
//                               cos(t) for odd j, every step in fp32 in the reference's order (the all-false mask makes the
//                               cumulative sums i + 1 and the table the same for every image).  One thread per element.
//   vitmi_add_rows_bcast        out[b, n, :] = x[b, n, :] + pos[n, :], pos fp32 [N, C], x and out bf16 or fp32.  A thread owns
//                               one 16-byte vector of the flat [B * N*C] tensor; where N*C is no multiple of the vector width
//                               a vector can straddle two images, so pos is then read per element at (flat index) mod N*C,
//                               and the last, partial vector of the tensor is moved element by element.
//   vitmi_ca_merge_fwd          x1[b, n, :] = x[b, n, :] + gamma1 * (n == 0 ? a[b, :] : l[b, n, :])
//   vitmi_ca_merge_bwd          from dx1, l, a, gamma1:  da[b, :] = gamma1 * dx1[b, 0, :] (operand dtype),
//                               dl[b, n, :] = n == 0 ? 0 : gamma1 * dx1[b, n, :] (fp32, STORED: the data-gradient products of
//                               the k / v and q projections are then accumulated onto it),
//                               dgamma1 = sum_b dx1[b, 0] a[b] + sum_{b, n >= 1} dx1[b, n] l[b, n] in two levels as
//                               vitmi_colsum_mul does: S = min(ceil(B*N1 / 4), 512) partial rows, wave w of workgroup y sums
//                               rows 4 y + w, 4 (y + S) + w, ..., the four waves are added in LDS, vitmi_reduce_rows folds.
//                               Every (row, vector) is visited by exactly one thread, which also writes its da / dl vector.
//   vitmi_ca_out_fwd            out[b, n, :] = n == 0 ? xc[b, :] + gamma2 * m[b, :] : 2 * xp[b, n, :].  xc: the normed CLS rows at
//                               a caller-given stride (row 0 of norm2's full output, or its compact [B, D] output when only
//                               the CLS row is normed); xp: the tensor that holds the patch rows (norm2's output, or x1).
//   vitmi_ca_out_bwd            dx2[b, n, :] = n == 0 ? G[b, 0, :] : 2 * G[b, n, :];  gm[b, :] = gamma2 * G[b, 0, :] (operand dtype)
//
// The XCABlock's junction (vitmi_ls_residual_ln_fwd) is a LayerNorm row kernel and lives in layernorm.hip.
#include "common.h"

namespace {

#include "bnrows.h"

constexpr int PF_HIDDEN = 32;
constexpr int GRID_CAP = 256 * 16;      // workgroups of a striding kernel, at most: sixteen per CU

// ------------------------------------------------------------------------------------------------ positional ---
template <typename T>
__global__ __launch_bounds__(NT) void posfourier_kernel(T* __restrict__ out, int Hp, int Wp, float temperature, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % (2 * PF_HIDDEN));
  const int64_t p = i / (2 * PF_HIDDEN);
  const int y = (int)(p / Wp), x = (int)(p - (int64_t)y * Wp);
  const bool is_y = c < PF_HIDDEN;
  const int j = is_y ? c : c - PF_HIDDEN;
  const float idx = (float)((is_y ? y : x) + 1);
  const float ext = (float)(is_y ? Hp : Wp) + 1e-6f;
  const float embed = idx / ext * 6.283185307179586f;
  const float dim_t = powf(temperature, (float)(2 * (j / 2)) / (float)PF_HIDDEN);
  const float t = embed / dim_t;
  out[i] = from_f32<T>((j & 1) ? cosf(t) : sinf(t));
}

template <typename T, bool ALIGNED>
__global__ __launch_bounds__(NT) void add_rows_bcast_kernel(const T* __restrict__ x, const float* __restrict__ pos,
                                                            T* __restrict__ out, int64_t NC, int64_t total) {
  constexpr int V = Vec<T>::N;
  const int64_t nvec = total / V;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * NT) {
    const int64_t f = i * V;
    float xv[V], pv[V];
    Vec<T>::load(x + f, xv);
    if (ALIGNED) {
      loadf<V>(pos + f % NC, pv);
    } else {
      int64_t r = f % NC;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        pv[e] = pos[r];
        r = r + 1 == NC ? 0 : r + 1;
      }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) xv[e] += pv[e];
    Vec<T>::store(out + f, xv);
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(total - nvec * V)) {     // the tensor's last, partial vector
    const int64_t f = nvec * V + threadIdx.x;
    out[f] = from_f32<T>(to_f32(x[f]) + pos[f % NC]);
  }
}

// ------------------------------------------------------------------------------------- class-attention glue ---
struct CaDims { int N1, D4; int64_t nvec; };      // D4 = D / 4 vectors per row, nvec = B * N1 * D4

template <typename T>
__global__ __launch_bounds__(NT) void ca_merge_fwd_kernel(const float* __restrict__ x, const T* __restrict__ a,
                                                          const T* __restrict__ l, const float* __restrict__ gamma1,
                                                          float* __restrict__ x1, CaDims d) {
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < d.nvec; i += (int64_t)gridDim.x * NT) {
    const int64_t row = i / d.D4;
    const int c = (int)(i - row * d.D4) * 4;
    const int64_t b = row / d.N1;
    const bool cls = row - b * d.N1 == 0;
    const int64_t D = (int64_t)d.D4 * 4;
    const f32x4 xv = load4<float>(x + row * D + c), g = load4<float>(gamma1 + c);
    const f32x4 br = cls ? load4<T>(a + b * D + c) : load4<T>(l + row * D + c);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = fmaf(g[e], br[e], xv[e]);
    store4<float>(x1 + row * D + c, o);
  }
}

// grid (ceil(D / 256), S): the colsum_mul decomposition, with the da / dl vectors written on the way
template <typename T>
__global__ __launch_bounds__(256) void ca_merge_bwd_kernel(const float* __restrict__ dx1, const T* __restrict__ l,
                                                           const T* __restrict__ a, const float* __restrict__ gamma1,
                                                           T* __restrict__ da, float* __restrict__ dl, float* __restrict__ part,
                                                           int64_t R, int N1, int64_t D) {
  __shared__ float red[4][256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t c0 = ((int64_t)blockIdx.x * 64 + lane) * 4;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (c0 < D) {
    const f32x4 g = load4<float>(gamma1 + c0);
    for (int64_t r = (int64_t)blockIdx.y * 4 + w; r < R; r += (int64_t)gridDim.y * 4) {
      const int64_t b = r / N1;
      const bool cls = r - b * N1 == 0;
      const f32x4 dv = load4<float>(dx1 + r * D + c0);
      const f32x4 br = cls ? load4<T>(a + b * D + c0) : load4<T>(l + r * D + c0);
      f32x4 s;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[e] = fmaf(dv[e], br[e], acc[e]);
        s[e] = g[e] * dv[e];
      }
      if (cls) {
        store4<T>(da + b * D + c0, s);
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        store4<float>(dl + r * D + c0, z);
      } else {
        store4<float>(dl + r * D + c0, s);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[w][lane * 4 + e] = acc[e];
  __syncthreads();
  if (w == 0 && c0 < D)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = lane * 4 + e;
      part[(int64_t)blockIdx.y * D + c0 + e] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void ca_out_fwd_kernel(const float* __restrict__ xc, int64_t xc_stride,
                                                        const float* __restrict__ xp, const T* __restrict__ m,
                                                        const float* __restrict__ gamma2, float* __restrict__ out, CaDims d) {
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < d.nvec; i += (int64_t)gridDim.x * NT) {
    const int64_t row = i / d.D4;
    const int c = (int)(i - row * d.D4) * 4;
    const int64_t b = row / d.N1;
    const int64_t D = (int64_t)d.D4 * 4;
    f32x4 o;
    if (row - b * d.N1 == 0) {
      const f32x4 xv = load4<float>(xc + b * xc_stride + c), g = load4<float>(gamma2 + c), mv = load4<T>(m + b * D + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = fmaf(g[e], mv[e], xv[e]);
    } else {
      const f32x4 xv = load4<float>(xp + row * D + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = 2.f * xv[e];
    }
    store4<float>(out + row * D + c, o);
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void ca_out_bwd_kernel(const float* __restrict__ G, const float* __restrict__ gamma2,
                                                        float* __restrict__ dx2, T* __restrict__ gm, CaDims d) {
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < d.nvec; i += (int64_t)gridDim.x * NT) {
    const int64_t row = i / d.D4;
    const int c = (int)(i - row * d.D4) * 4;
    const int64_t b = row / d.N1;
    const int64_t D = (int64_t)d.D4 * 4;
    f32x4 gv = load4<float>(G + row * D + c);
    if (row - b * d.N1 == 0) {
      const f32x4 g = load4<float>(gamma2 + c);
      f32x4 s;
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = g[e] * gv[e];
      store4<T>(gm + b * D + c, s);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = 2.f * gv[e];
    }
    store4<float>(dx2 + row * D + c, gv);
  }
}

// ---------------------------------------------------------------------------------------------------- dispatch ---
bool dtype_ok(int dtype) { return dtype == VITMI_BF16 || dtype == VITMI_F32; }

bool ca_shape_ok(int64_t B, int64_t N1, int64_t D) {
  return B >= 1 && N1 >= 2 && N1 < (1 << 20) && D >= 8 && D % 8 == 0 && D < (1 << 20) && B * N1 < (1ll << 31);
}

int ca_check(const char* who, int dtype, int64_t B, int64_t N1, int64_t D) {
  VITMI_REQUIRE(dtype_ok(dtype), VITMI_E_DTYPE, "%s: the operand dtype must be bf16 or fp32", who);
  VITMI_REQUIRE(ca_shape_ok(B, N1, D), VITMI_E_SHAPE,
                "%s: B = %lld, N1 = %lld, D = %lld: B >= 1, N1 >= 2 (a CLS row and at least one patch row), D a multiple of 8, "
                "B*N1 < 2^31",
                who, (long long)B, (long long)N1, (long long)D);
  return 0;
}

CaDims ca_dims(int64_t B, int64_t N1, int64_t D) {
  CaDims d;
  d.N1 = (int)N1; d.D4 = (int)(D / 4); d.nvec = B * N1 * (D / 4);
  return d;
}

unsigned stride_grid(int64_t units) {
  const int64_t blocks = (units + NT - 1) / NT;
  return (unsigned)(blocks < 1 ? 1 : blocks < GRID_CAP ? blocks : GRID_CAP);
}

}  // namespace

extern "C" int vitmi_posfourier_supported(int dtype, int64_t Hp, int64_t Wp, int64_t hidden_dim) {
  return dtype_ok(dtype) && hidden_dim == PF_HIDDEN && Hp >= 1 && Wp >= 1 && Hp < (1 << 15) && Wp < (1 << 15);
}

extern "C" int vitmi_posfourier_features(void* out, int dtype, int64_t Hp, int64_t Wp, int64_t hidden_dim, float temperature,
                                         void* stream) {
  VITMI_REQUIRE(dtype_ok(dtype), VITMI_E_DTYPE, "posfourier_features: the table's dtype must be bf16 or fp32");
  VITMI_REQUIRE(hidden_dim == PF_HIDDEN, VITMI_E_SHAPE, "posfourier_features: hidden_dim = %lld is not built (only %d is)",
                (long long)hidden_dim, PF_HIDDEN);
  VITMI_REQUIRE(Hp >= 1 && Wp >= 1 && Hp < (1 << 15) && Wp < (1 << 15), VITMI_E_SHAPE,
                "posfourier_features: the grid %lld x %lld must be at least 1 x 1 (below 2^15 a side)", (long long)Hp, (long long)Wp);
  VITMI_REQUIRE(temperature > 0.f, VITMI_E_BADARG, "posfourier_features: the temperature must be positive");
  VITMI_REQUIRE(out && is_aligned(out, dtype_size(dtype)), VITMI_E_BADARG, "posfourier_features: null or misaligned out");
  const int64_t total = Hp * Wp * 2 * PF_HIDDEN;
  const dim3 grid((unsigned)((total + NT - 1) / NT));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == VITMI_BF16)
    hipLaunchKernelGGL((posfourier_kernel<bf16>), grid, dim3(NT), 0, s, (bf16*)out, (int)Hp, (int)Wp, temperature, total);
  else
    hipLaunchKernelGGL((posfourier_kernel<float>), grid, dim3(NT), 0, s, (float*)out, (int)Hp, (int)Wp, temperature, total);
  return vitmi_check_launch("posfourier_kernel");
}

extern "C" int vitmi_add_rows_bcast_supported(int dtype, int64_t B, int64_t N, int64_t C) {
  return dtype_ok(dtype) && B >= 1 && N >= 1 && C >= 1 && N * C < (1ll << 31) && B < (1ll << 31) && B * N * C < (1ll << 40);
}

extern "C" int vitmi_add_rows_bcast(const void* x, const float* pos, void* out, int dtype, int64_t B, int64_t N, int64_t C,
                                    void* stream) {
  VITMI_REQUIRE(dtype_ok(dtype), VITMI_E_DTYPE, "add_rows_bcast: x and out must be bf16 or fp32");
  VITMI_REQUIRE(vitmi_add_rows_bcast_supported(dtype, B, N, C), VITMI_E_SHAPE,
                "add_rows_bcast: B = %lld, N = %lld, C = %lld: every extent at least 1, N*C < 2^31, B*N*C < 2^40", (long long)B,
                (long long)N, (long long)C);
  VITMI_REQUIRE(x && pos && out, VITMI_E_BADARG, "add_rows_bcast: null pointer");
  VITMI_REQUIRE(is_aligned(x, 16) && is_aligned(out, 16) && is_aligned(pos, 16), VITMI_E_ALIGN,
                "add_rows_bcast: x, pos and out must be 16-B aligned");
  const int64_t NC = N * C, total = B * NC;
  const int V = dtype == VITMI_BF16 ? 8 : 4;
  const bool aligned = NC % V == 0;
  const dim3 grid(stride_grid(total / V));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define ARB(T, AL) hipLaunchKernelGGL((add_rows_bcast_kernel<T, AL>), grid, dim3(NT), 0, s, (const T*)x, pos, (T*)out, NC, total)
  if (dtype == VITMI_BF16) { if (aligned) ARB(bf16, true); else ARB(bf16, false); }
  else { if (aligned) ARB(float, true); else ARB(float, false); }
#undef ARB
  return vitmi_check_launch("add_rows_bcast_kernel");
}

extern "C" int vitmi_ca_glue_supported(int dtype, int64_t B, int64_t N1, int64_t D) {
  return dtype_ok(dtype) && ca_shape_ok(B, N1, D);
}

extern "C" int vitmi_ca_merge_fwd(const float* x, const void* a, const void* l, const float* gamma1, float* x1, int dtype,
                                  int64_t B, int64_t N1, int64_t D, void* stream) {
  if (int rc = ca_check("ca_merge_fwd", dtype, B, N1, D)) return rc;
  VITMI_REQUIRE(x && a && l && gamma1 && x1, VITMI_E_BADARG, "ca_merge_fwd: null pointer");
  VITMI_REQUIRE(is_aligned(x, 16) && is_aligned(a, 16) && is_aligned(l, 16) && is_aligned(gamma1, 16) && is_aligned(x1, 16),
                VITMI_E_ALIGN, "ca_merge_fwd: x, a, l, gamma1 and x1 must be 16-B aligned");
  const CaDims d = ca_dims(B, N1, D);
  const dim3 grid(stride_grid(d.nvec));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == VITMI_BF16)
    hipLaunchKernelGGL((ca_merge_fwd_kernel<bf16>), grid, dim3(NT), 0, s, x, (const bf16*)a, (const bf16*)l, gamma1, x1, d);
  else
    hipLaunchKernelGGL((ca_merge_fwd_kernel<float>), grid, dim3(NT), 0, s, x, (const float*)a, (const float*)l, gamma1, x1, d);
  return vitmi_check_launch("ca_merge_fwd_kernel");
}

extern "C" size_t vitmi_ca_merge_bwd_workspace(int64_t B, int64_t N1, int64_t D) {
  if (!ca_shape_ok(B, N1, D)) return 0;
  return (size_t)colsum_splits(B * N1) * (size_t)D * sizeof(float);
}

extern "C" int vitmi_ca_merge_bwd(const float* dx1, const void* l, const void* a, const float* gamma1, void* da, float* dl,
                                  float* dgamma1, int dtype, int64_t B, int64_t N1, int64_t D, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  if (int rc = ca_check("ca_merge_bwd", dtype, B, N1, D)) return rc;
  VITMI_REQUIRE(dx1 && l && a && gamma1 && da && dl && dgamma1, VITMI_E_BADARG, "ca_merge_bwd: null pointer");
  VITMI_REQUIRE(is_aligned(dx1, 16) && is_aligned(l, 16) && is_aligned(a, 16) && is_aligned(gamma1, 16) && is_aligned(da, 16) &&
                    is_aligned(dl, 16) && is_aligned(dgamma1, 4),
                VITMI_E_ALIGN, "ca_merge_bwd: dx1, l, a, gamma1, da and dl must be 16-B aligned");
  VITMI_REQUIRE(workspace && is_aligned(workspace, 16) && workspace_bytes >= vitmi_ca_merge_bwd_workspace(B, N1, D),
                VITMI_E_WORKSPACE, "ca_merge_bwd: workspace missing, not 16-B aligned or smaller than vitmi_ca_merge_bwd_workspace");
  const int64_t R = B * N1;
  const int S = colsum_splits(R);
  float* part = reinterpret_cast<float*>(workspace);
  const dim3 grid((unsigned)((D + 255) / 256), (unsigned)S);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == VITMI_BF16)
    hipLaunchKernelGGL((ca_merge_bwd_kernel<bf16>), grid, dim3(256), 0, s, dx1, (const bf16*)l, (const bf16*)a, gamma1, (bf16*)da,
                       dl, part, R, (int)N1, D);
  else
    hipLaunchKernelGGL((ca_merge_bwd_kernel<float>), grid, dim3(256), 0, s, dx1, (const float*)l, (const float*)a, gamma1,
                       (float*)da, dl, part, R, (int)N1, D);
  if (int rc = vitmi_check_launch("ca_merge_bwd_kernel")) return rc;
  return vitmi_reduce_rows(part, S, D, D, dgamma1, s);
}

extern "C" int vitmi_ca_out_fwd(const float* xc, int64_t xc_stride, const float* xp, const void* m, const float* gamma2,
                                float* out, int dtype, int64_t B, int64_t N1, int64_t D, void* stream) {
  if (int rc = ca_check("ca_out_fwd", dtype, B, N1, D)) return rc;
  VITMI_REQUIRE(xc && xp && m && gamma2 && out, VITMI_E_BADARG, "ca_out_fwd: null pointer");
  VITMI_REQUIRE(xc_stride >= D && xc_stride % 4 == 0, VITMI_E_ALIGN, "ca_out_fwd: xc_stride must be a multiple of 4 and at least D");
  VITMI_REQUIRE(is_aligned(xc, 16) && is_aligned(xp, 16) && is_aligned(m, 16) && is_aligned(gamma2, 16) && is_aligned(out, 16),
                VITMI_E_ALIGN, "ca_out_fwd: xc, xp, m, gamma2 and out must be 16-B aligned");
  const CaDims d = ca_dims(B, N1, D);
  const dim3 grid(stride_grid(d.nvec));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == VITMI_BF16)
    hipLaunchKernelGGL((ca_out_fwd_kernel<bf16>), grid, dim3(NT), 0, s, xc, xc_stride, xp, (const bf16*)m, gamma2, out, d);
  else
    hipLaunchKernelGGL((ca_out_fwd_kernel<float>), grid, dim3(NT), 0, s, xc, xc_stride, xp, (const float*)m, gamma2, out, d);
  return vitmi_check_launch("ca_out_fwd_kernel");
}

extern "C" int vitmi_ca_out_bwd(const float* G, const float* gamma2, float* dx2, void* gm, int dtype, int64_t B, int64_t N1,
                                int64_t D, void* stream) {
  if (int rc = ca_check("ca_out_bwd", dtype, B, N1, D)) return rc;
  VITMI_REQUIRE(G && gamma2 && dx2 && gm, VITMI_E_BADARG, "ca_out_bwd: null pointer");
  VITMI_REQUIRE(is_aligned(G, 16) && is_aligned(gamma2, 16) && is_aligned(dx2, 16) && is_aligned(gm, 16), VITMI_E_ALIGN,
                "ca_out_bwd: G, gamma2, dx2 and gm must be 16-B aligned");
  const CaDims d = ca_dims(B, N1, D);
  const dim3 grid(stride_grid(d.nvec));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == VITMI_BF16)
    hipLaunchKernelGGL((ca_out_bwd_kernel<bf16>), grid, dim3(NT), 0, s, G, gamma2, dx2, (bf16*)gm, d);
  else
    hipLaunchKernelGGL((ca_out_bwd_kernel<float>), grid, dim3(NT), 0, s, G, gamma2, dx2, (float*)gm, d);
  return vitmi_check_launch("ca_out_bwd_kernel");
}
