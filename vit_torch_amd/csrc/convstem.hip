// XCiT's ConvPatchEmbed stages (models/xcit.py:58-108 of the reference): Conv2d(3 x 3, stride 2, padding 1, no bias),
// BatchNorm2d, and GELU between the stages, on token-major activations [B, H*W, C] with C contiguous.  The convolution is
// a gather into an im2col matrix and a product on the existing GEMM kernels (no GEMM lives here):
//   col [B*Ho*Wo, ld], Ho = ceil(H/2), Wo = ceil(W/2):  col[(b,oy,ox), c*9 + i*3 + j] = x[b, 2oy-1+i, 2ox-1+j, c], 0 outside
// which is vitmi_patchify's K order, so a conv weight [Cout, Cin, 3, 3] in its own memory is the k-major B operand.
//
//   vitmi_conv3s2_im2col   the gather.  Token-major form: a thread owns (one col row, 8 channels): it reads the nine taps
//                          as 16-byte channel vectors (coalesced over the channel groups of a pixel), transposes the 9 x 8
//                          block in registers (every index is a compile-time constant) and stores the 72 contiguous
//                          elements [72 g, 72 g + 72) of its col row as 16-byte vectors: no LDS is needed for wide stores,
//                          because 8 channels x 9 taps is a whole number of 16-byte vectors in both dtypes.  Image form
//                          (fp32 NCHW or channels_last through element strides, Cin = 3): a thread owns one col row, reads
//                          its 27 values and stores the row (27 values, then zeros up to ld) as 16-byte vectors.  A pure copy
//                          or cast.  Columns [9 Cin, ld) are written as zeros.
//   vitmi_conv3s2_col2im   the transpose, as a gather: a thread owns (one pixel, 8 channels) and sums the 1, 2 or 4 entries
//                          of dcol that read it, in fp32, rows (i) outer and columns (j) inner, earlier output position
//                          first; one 16-byte store.  No atomics.  Its reads are element-wide (stride 9 inside a 72-element
//                          segment): each segment is read by nine pixels and stays in L1 / L2.
//   vitmi_bn_act_fwd/_bwd  BatchNorm over the rows of y [M, C] as stored, with an optional GELU after it.  The decomposition
//                          and the statistics are bnrows.h's, shared with lpi.hip.
//                            forward, training: bn_stat_kernel (y -> per-chunk (mean, M2)), stat_kernel, bn_apply_kernel
//                            forward, eval:     eval_stat_kernel, bn_apply_kernel; no buffer is touched
//                            backward:          bn_red_kernel (dout, y -> per-chunk dbeta | dgamma), vitmi_reduce_rows x 2,
//                                               bn_dy_kernel (dout, y -> dy).  z is recomputed; z and out are not kept.
//   vitmi_conv3s2_wcopy    dst[r, c] = src[r, c] for c < cols, 0 for cols <= c < dst_cols: the [Cout, 32] image of the first
//                          stage's [Cout, 27] weight, and the first 27 columns of its [Cout, 32] gradient product back.
#include "common.h"

namespace {

#include "bnrows.h"

// ------------------------------------------------------------------------------------------------ the gathers ---
struct ConvDims { int H, W, Ho, Wo, C; int64_t ld, units; };

// token-major: unit = (col row m, channel group g of 8); G = C / 8
template <typename T>
__global__ __launch_bounds__(NT) void im2col_kernel(const T* __restrict__ x, T* __restrict__ col, ConvDims d) {
  constexpr int V = Vec<T>::N, NV = 8 / V;              // NV 16-byte vectors per 8 channels
  const int G = d.C >> 3;
  const int64_t u = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (u >= d.units) return;
  const int64_t m = u / G;
  const int g = (int)(u - m * G);
  const int HoWo = d.Ho * d.Wo;
  const int64_t b = m / HoWo;
  const int r = (int)(m - b * HoWo), oy = r / d.Wo, ox = r - oy * d.Wo;
  float v[9][8];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int y = 2 * oy - 1 + i, xx = 2 * ox - 1 + j;
      if ((unsigned)y < (unsigned)d.H && (unsigned)xx < (unsigned)d.W) {
        const T* src = x + ((b * d.H + y) * d.W + xx) * d.C + g * 8;
#pragma unroll
        for (int h = 0; h < NV; ++h) Vec<T>::load(src + h * V, v[i * 3 + j] + h * V);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[i * 3 + j][e] = 0.f;
      }
    }
  T* dst = col + m * d.ld + g * 72;
#pragma unroll
  for (int q = 0; q < 72 / V; ++q) {                    // element o = e * 9 + t of the segment
    float w[V];
#pragma unroll
    for (int k = 0; k < V; ++k) w[k] = v[(q * V + k) % 9][(q * V + k) / 9];
    Vec<T>::store(dst + q * V, w);
  }
  if (g == 0) {                                          // the pad columns of this row
    float z[V];
#pragma unroll
    for (int k = 0; k < V; ++k) z[k] = 0.f;
    for (int64_t c = 9 * (int64_t)d.C; c < d.ld; c += V) Vec<T>::store(col + m * d.ld + c, z);
  }
}

// image form: fp32 x with element strides, 3 channels; unit = col row m
template <typename T>
__global__ __launch_bounds__(NT) void im2col_image_kernel(const float* __restrict__ x, int64_t sb, int64_t sc, int64_t sh,
                                                          int64_t sw, T* __restrict__ col, ConvDims d) {
  constexpr int V = Vec<T>::N;
  const int64_t m = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (m >= d.units) return;
  const int HoWo = d.Ho * d.Wo;
  const int64_t b = m / HoWo;
  const int r = (int)(m - b * HoWo), oy = r / d.Wo, ox = r - oy * d.Wo;
  float v[32];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int y = 2 * oy - 1 + i, xx = 2 * ox - 1 + j;
        const bool in = (unsigned)y < (unsigned)d.H && (unsigned)xx < (unsigned)d.W;
        v[c * 9 + i * 3 + j] = in ? x[b * sb + c * sc + y * sh + xx * sw] : 0.f;
      }
#pragma unroll
  for (int k = 27; k < 32; ++k) v[k] = 0.f;
  T* dst = col + m * d.ld;
#pragma unroll
  for (int q = 0; q < 32 / V; ++q) Vec<T>::store(dst + q * V, v + q * V);
  float z[V];
#pragma unroll
  for (int k = 0; k < V; ++k) z[k] = 0.f;
  for (int64_t c = 32; c < d.ld; c += V) Vec<T>::store(dst + c, z);
}

// unit = (pixel p, channel group g of 8)
template <typename T>
__global__ __launch_bounds__(NT) void col2im_kernel(const T* __restrict__ dcol, T* __restrict__ dx, ConvDims d) {
  constexpr int V = Vec<T>::N, NV = 8 / V;
  const int G = d.C >> 3;
  const int64_t u = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (u >= d.units) return;
  const int64_t p = u / G;
  const int g = (int)(u - p * G);
  const int HW = d.H * d.W;
  const int64_t b = p / HW;
  const int r = (int)(p - b * HW), y = r / d.W, xx = r - y * d.W;
  // the (output coordinate, tap) pairs that read coordinate y: even: (y/2, 1); odd: ((y-1)/2, 2) then ((y+1)/2, 0) if inside
  int oys[2], is[2], oxs[2], js[2];
  const int ny = (y & 1) ? ((y + 1) / 2 < d.Ho ? 2 : 1) : 1, nx = (xx & 1) ? ((xx + 1) / 2 < d.Wo ? 2 : 1) : 1;
  oys[0] = y >> 1;          is[0] = (y & 1) ? 2 : 1;
  oys[1] = (y + 1) >> 1;    is[1] = 0;
  oxs[0] = xx >> 1;         js[0] = (xx & 1) ? 2 : 1;
  oxs[1] = (xx + 1) >> 1;   js[1] = 0;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (a < ny && c < nx) {
        const int64_t m = (b * d.Ho + oys[a]) * d.Wo + oxs[c];
        const T* src = dcol + m * d.ld + g * 72 + is[a] * 3 + js[c];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += to_f32(src[e * 9]);
      }
    }
  T* dst = dx + p * d.C + g * 8;
#pragma unroll
  for (int h = 0; h < NV; ++h) Vec<T>::store(dst + h * V, acc + h * V);
}

template <typename T>
__global__ __launch_bounds__(NT) void wcopy_kernel(const T* __restrict__ src, int64_t src_ld, T* __restrict__ dst, int64_t dst_ld,
                                                   int64_t rows, int cols, int dst_cols) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= rows * dst_cols) return;
  const int64_t r = i / dst_cols;
  const int c = (int)(i - r * dst_cols);
  dst[r * dst_ld + c] = c < cols ? src[r * src_ld + c] : from_f32<T>(0.f);
}

// ------------------------------------------------------------------------------------------------ bn + act ---
// the workgroup's (mean, M2) of its rows of y to part[chunk][2][C] (double)
template <typename T>
__global__ __launch_bounds__(NT) void bn_stat_kernel(const T* __restrict__ y, double* __restrict__ part, RowDims d) {
  constexpr int V = Vec<T>::N;
  __shared__ __attribute__((aligned(16))) float red[2 * NT * V];
  __shared__ float cnt[NT];
  Place pc;
  pc.init<V>(d);
  float mean[V], m2[V];
#pragma unroll
  for (int v = 0; v < V; ++v) { mean[v] = 0.f; m2[v] = 0.f; }
  float n = 0.f;
  if (pc.active) {
    for (int64_t p = pc.p_begin + pc.pl; p < pc.p_end; p += pc.PL) {
      float yv[V];
      Vec<T>::load(y + p * d.C + pc.c0, yv);
      n += 1.f;
      welford_step<V>(yv, n, mean, m2);
    }
  }
  welford_block_store<V>(red, cnt, mean, m2, n, pc, part, d.C);
}

// out = act((y - mean) rstd gamma + beta)
template <typename T, bool GELU>
__global__ __launch_bounds__(NT) void bn_apply_kernel(const T* __restrict__ y, const float* __restrict__ stat,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      T* __restrict__ out, RowDims d) {
  constexpr int V = Vec<T>::N;
  Place pc;
  pc.init<V>(d);
  if (!pc.active) return;
  Norm<V> nm;
  nm.load(stat, gamma, beta, d.C, pc.c0);
  for (int64_t p = pc.p_begin + pc.pl; p < pc.p_end; p += pc.PL) {
    float yv[V];
    Vec<T>::load(y + p * d.C + pc.c0, yv);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const float z = fmaf((yv[v] - nm.mean[v]) * nm.rstd[v], nm.gamma[v], nm.beta[v]);
      yv[v] = GELU ? gelu_erf(z) : z;
    }
    Vec<T>::store(out + p * d.C + pc.c0, yv);
  }
}

// partial row of the chunk: dbeta [C] | dgamma [C]
template <typename T, bool GELU>
__global__ __launch_bounds__(NT) void bn_red_kernel(const T* __restrict__ dout, const T* __restrict__ y,
                                                    const float* __restrict__ stat, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, float* __restrict__ part, RowDims d) {
  constexpr int V = Vec<T>::N;
  __shared__ __attribute__((aligned(16))) float red[NT * V];
  Place pc;
  pc.init<V>(d);
  float dbeta[V], dgamma[V];
#pragma unroll
  for (int v = 0; v < V; ++v) dbeta[v] = dgamma[v] = 0.f;
  if (pc.active) {
    Norm<V> nm;
    nm.load(stat, gamma, beta, d.C, pc.c0);
    for (int64_t p = pc.p_begin + pc.pl; p < pc.p_end; p += pc.PL) {
      float yv[V], dv[V];
      Vec<T>::load(y + p * d.C + pc.c0, yv);
      Vec<T>::load(dout + p * d.C + pc.c0, dv);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const float yh = (yv[v] - nm.mean[v]) * nm.rstd[v];
        const float dz = GELU ? dv[v] * dgelu_erf(fmaf(yh, nm.gamma[v], nm.beta[v])) : dv[v];
        dbeta[v] += dz;
        dgamma[v] = fmaf(dz, yh, dgamma[v]);
      }
    }
  }
  float* row = part + (int64_t)blockIdx.x * 2 * d.C;
  lane_sum_store<V>(red, dbeta, pc, row + pc.c_base, 1, d.C);
  lane_sum_store<V>(red, dgamma, pc, row + d.C + pc.c_base, 1, d.C);
}

// dy = gamma rstd (dz - dbeta/M - yh dgamma/M)   (eval: gamma rstd dz)
template <typename T, bool GELU, bool TRAIN>
__global__ __launch_bounds__(NT) void bn_dy_kernel(const T* __restrict__ dout, const T* __restrict__ y,
                                                   const float* __restrict__ stat, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, const float* __restrict__ dgamma,
                                                   const float* __restrict__ dbeta, T* __restrict__ dy, RowDims d) {
  constexpr int V = Vec<T>::N;
  Place pc;
  pc.init<V>(d);
  if (!pc.active) return;
  Norm<V> nm;
  nm.load(stat, gamma, beta, d.C, pc.c0);
  float gr[V], mdz[V], mdzy[V];
  loadf<V>(dbeta + pc.c0, mdz);
  loadf<V>(dgamma + pc.c0, mdzy);
  const float invM = 1.f / (float)d.M;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    gr[v] = nm.gamma[v] * nm.rstd[v];
    mdz[v] = TRAIN ? mdz[v] * invM : 0.f;
    mdzy[v] = TRAIN ? mdzy[v] * invM : 0.f;
  }
  for (int64_t p = pc.p_begin + pc.pl; p < pc.p_end; p += pc.PL) {
    float yv[V], dv[V];
    Vec<T>::load(y + p * d.C + pc.c0, yv);
    Vec<T>::load(dout + p * d.C + pc.c0, dv);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const float yh = (yv[v] - nm.mean[v]) * nm.rstd[v];
      const float dz = GELU ? dv[v] * dgelu_erf(fmaf(yh, nm.gamma[v], nm.beta[v])) : dv[v];
      dv[v] = gr[v] * (TRAIN ? dz - mdz[v] - yh * mdzy[v] : dz);
    }
    Vec<T>::store(dy + p * d.C + pc.c0, dv);
  }
}

// ---------------------------------------------------------------------------------------------------- dispatch ---
bool dtype_ok(int dtype) { return dtype == VITMI_BF16 || dtype == VITMI_F32; }

RowDims rows_of(const Geo& g, int64_t C) {
  RowDims d;
  d.C = (int)C; d.chunk = g.chunk; d.gt_log2 = g.gt_log2; d.M = g.M;
  return d;
}

int check_conv(const char* who, int dtype, int image_form, int64_t B, int64_t H, int64_t W, int64_t C, int64_t ld) {
  VITMI_REQUIRE(dtype_ok(dtype), VITMI_E_DTYPE, "%s: the compute dtype must be bf16 or fp32", who);
  VITMI_REQUIRE(B >= 1 && H >= 1 && W >= 1 && H < (1 << 15) && W < (1 << 15) && B < (1ll << 31) && B * H * W < (1ll << 31),
                VITMI_E_SHAPE, "%s: B = %lld, H = %lld, W = %lld: every extent must be at least 1 (B*H*W < 2^31)", who,
                (long long)B, (long long)H, (long long)W);
  if (image_form)
    VITMI_REQUIRE(C == 3, VITMI_E_SHAPE, "%s: the image form takes 3 channels (got %lld)", who, (long long)C);
  else
    VITMI_REQUIRE(C >= 8 && C % 8 == 0 && C < (1 << 20), VITMI_E_SHAPE,
                  "%s: C = %lld must be a multiple of 8 (below 2^20) in the token-major form", who, (long long)C);
  VITMI_REQUIRE(ld >= 9 * C && ld % 8 == 0 && ld < (1ll << 31), VITMI_E_SHAPE,
                "%s: ld = %lld must be a multiple of 8 and at least 9*C = %lld", who, (long long)ld, (long long)(9 * C));
  return 0;
}

ConvDims conv_dims(int64_t H, int64_t W, int64_t C, int64_t ld, int64_t units) {
  ConvDims d;
  d.H = (int)H; d.W = (int)W; d.Ho = (int)((H + 1) / 2); d.Wo = (int)((W + 1) / 2); d.C = (int)C; d.ld = ld; d.units = units;
  return d;
}

int check_bn(const char* who, int dtype, int64_t M, int64_t C, int training) {
  VITMI_REQUIRE(dtype_ok(dtype), VITMI_E_DTYPE, "%s: activations must be bf16 or fp32", who);
  VITMI_REQUIRE(C >= 8 && C % 8 == 0 && C < (1 << 20), VITMI_E_SHAPE, "%s: C = %lld must be a multiple of 8 (below 2^20)", who,
                (long long)C);
  VITMI_REQUIRE(M >= 1 && M < (1ll << 31), VITMI_E_SHAPE, "%s: M = %lld rows: at least 1, below 2^31", who, (long long)M);
  VITMI_REQUIRE(!training || M > 1, VITMI_E_SHAPE,
                "%s: training needs more than one row per channel (M = 1): the batch variance is undefined", who);
  return 0;
}

template <typename T>
int bn_fwd(const T* y, const float* gamma, const float* beta, float* rmean, float* rvar, int64_t* nbt, float* stat, T* out,
           int gelu, int training, float momentum, float eps, const Geo& g, const RowDims& d, double* part, hipStream_t s) {
  const dim3 grid((unsigned)g.nch, (unsigned)g.tiles), cgrid((unsigned)((d.C + NT - 1) / NT));
  if (training) {
    hipLaunchKernelGGL((bn_stat_kernel<T>), grid, dim3(NT), 0, s, y, part, d);
    if (int rc = vitmi_check_launch("bn_act bn_stat_kernel")) return rc;
    hipLaunchKernelGGL(stat_kernel, cgrid, dim3(NT), 0, s, (const double*)part, g.nch, d, momentum, eps, stat, rmean, rvar, nbt);
    if (int rc = vitmi_check_launch("bn_act stat_kernel")) return rc;
  } else {
    hipLaunchKernelGGL(eval_stat_kernel, cgrid, dim3(NT), 0, s, (const float*)rmean, (const float*)rvar, d.C, eps, stat);
    if (int rc = vitmi_check_launch("bn_act eval_stat_kernel")) return rc;
  }
  if (gelu)
    hipLaunchKernelGGL((bn_apply_kernel<T, true>), grid, dim3(NT), 0, s, y, (const float*)stat, gamma, beta, out, d);
  else
    hipLaunchKernelGGL((bn_apply_kernel<T, false>), grid, dim3(NT), 0, s, y, (const float*)stat, gamma, beta, out, d);
  return vitmi_check_launch("bn_act bn_apply_kernel");
}

template <typename T, bool GELU>
int bn_bwd(const T* dout, const T* y, const float* stat, const float* gamma, const float* beta, T* dy, float* dgamma,
           float* dbeta, int training, const Geo& g, const RowDims& d, float* part, hipStream_t s) {
  const dim3 grid((unsigned)g.nch, (unsigned)g.tiles);
  const int C = d.C;
  hipLaunchKernelGGL((bn_red_kernel<T, GELU>), grid, dim3(NT), 0, s, dout, y, stat, gamma, beta, part, d);
  if (int rc = vitmi_check_launch("bn_act bn_red_kernel")) return rc;
  if (int rc = vitmi_reduce_rows(part, g.nch, C, 2 * (int64_t)C, dbeta, s)) return rc;
  if (int rc = vitmi_reduce_rows(part + C, g.nch, C, 2 * (int64_t)C, dgamma, s)) return rc;
  if (training)
    hipLaunchKernelGGL((bn_dy_kernel<T, GELU, true>), grid, dim3(NT), 0, s, dout, y, stat, gamma, beta, (const float*)dgamma,
                       (const float*)dbeta, dy, d);
  else
    hipLaunchKernelGGL((bn_dy_kernel<T, GELU, false>), grid, dim3(NT), 0, s, dout, y, stat, gamma, beta, (const float*)dgamma,
                       (const float*)dbeta, dy, d);
  return vitmi_check_launch("bn_act bn_dy_kernel");
}

}  // namespace

extern "C" int vitmi_conv3s2_supported(int dtype, int image_form, int64_t B, int64_t H, int64_t W, int64_t C, int64_t ld) {
  return dtype_ok(dtype) && B >= 1 && H >= 1 && W >= 1 && H < (1 << 15) && W < (1 << 15) && B < (1ll << 31) &&
         B * H * W < (1ll << 31) && (image_form ? C == 3 : (C >= 8 && C % 8 == 0 && C < (1 << 20))) && ld >= 9 * C &&
         ld % 8 == 0 && ld < (1ll << 31);
}

extern "C" int vitmi_conv3s2_im2col(const void* x, int image_form, int64_t sb, int64_t sc, int64_t sh, int64_t sw, void* col,
                                    int dtype, int64_t ld, int64_t B, int64_t H, int64_t W, int64_t C, void* stream) {
  if (int rc = check_conv("conv3s2_im2col", dtype, image_form, B, H, W, C, ld)) return rc;
  VITMI_REQUIRE(x && col, VITMI_E_BADARG, "conv3s2_im2col: null pointer");
  VITMI_REQUIRE(is_aligned(col, 16) && is_aligned(x, image_form ? 4 : 16), VITMI_E_ALIGN,
                "conv3s2_im2col: col (and a token-major x) must be 16-B aligned");
  VITMI_REQUIRE(!image_form || (sb >= 0 && sc >= 0 && sh >= 0 && sw >= 0), VITMI_E_BADARG,
                "conv3s2_im2col: the image's strides must not be negative");
  const int64_t M = B * ((H + 1) / 2) * ((W + 1) / 2);
  const int64_t units = image_form ? M : M * (C / 8);
  const ConvDims d = conv_dims(H, W, C, ld, units);
  const int64_t blocks = (units + NT - 1) / NT;
  VITMI_REQUIRE(blocks < (1ll << 31), VITMI_E_SHAPE, "conv3s2_im2col: too many workgroups");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (image_form) {
    if (dtype == VITMI_BF16)
      hipLaunchKernelGGL((im2col_image_kernel<bf16>), dim3((unsigned)blocks), dim3(NT), 0, s, (const float*)x, sb, sc, sh, sw,
                         (bf16*)col, d);
    else
      hipLaunchKernelGGL((im2col_image_kernel<float>), dim3((unsigned)blocks), dim3(NT), 0, s, (const float*)x, sb, sc, sh, sw,
                         (float*)col, d);
    return vitmi_check_launch("conv3s2 im2col_image_kernel");
  }
  if (dtype == VITMI_BF16)
    hipLaunchKernelGGL((im2col_kernel<bf16>), dim3((unsigned)blocks), dim3(NT), 0, s, (const bf16*)x, (bf16*)col, d);
  else
    hipLaunchKernelGGL((im2col_kernel<float>), dim3((unsigned)blocks), dim3(NT), 0, s, (const float*)x, (float*)col, d);
  return vitmi_check_launch("conv3s2 im2col_kernel");
}

extern "C" int vitmi_conv3s2_col2im(const void* dcol, int64_t ld, void* dx, int dtype, int64_t B, int64_t H, int64_t W,
                                    int64_t C, void* stream) {
  if (int rc = check_conv("conv3s2_col2im", dtype, 0, B, H, W, C, ld)) return rc;
  VITMI_REQUIRE(dcol && dx, VITMI_E_BADARG, "conv3s2_col2im: null pointer");
  VITMI_REQUIRE(is_aligned(dcol, 16) && is_aligned(dx, 16), VITMI_E_ALIGN, "conv3s2_col2im: dcol and dx must be 16-B aligned");
  const int64_t units = B * H * W * (C / 8);
  const ConvDims d = conv_dims(H, W, C, ld, units);
  const int64_t blocks = (units + NT - 1) / NT;
  VITMI_REQUIRE(blocks < (1ll << 31), VITMI_E_SHAPE, "conv3s2_col2im: too many workgroups");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == VITMI_BF16)
    hipLaunchKernelGGL((col2im_kernel<bf16>), dim3((unsigned)blocks), dim3(NT), 0, s, (const bf16*)dcol, (bf16*)dx, d);
  else
    hipLaunchKernelGGL((col2im_kernel<float>), dim3((unsigned)blocks), dim3(NT), 0, s, (const float*)dcol, (float*)dx, d);
  return vitmi_check_launch("conv3s2 col2im_kernel");
}

extern "C" int vitmi_conv3s2_wcopy(const void* src, int64_t src_ld, void* dst, int64_t dst_ld, int dtype, int64_t rows,
                                   int64_t cols, int64_t dst_cols, void* stream) {
  VITMI_REQUIRE(dtype_ok(dtype), VITMI_E_DTYPE, "conv3s2_wcopy: the dtype must be bf16 or fp32");
  VITMI_REQUIRE(src && dst, VITMI_E_BADARG, "conv3s2_wcopy: null pointer");
  VITMI_REQUIRE(rows >= 1 && cols >= 1 && cols <= dst_cols && dst_cols <= dst_ld && cols <= src_ld && dst_ld < (1 << 20) &&
                    src_ld < (1 << 20) && rows < (1 << 20) && rows * dst_cols < (1ll << 31),
                VITMI_E_SHAPE,
                "conv3s2_wcopy: need 1 <= cols <= dst_cols <= dst_ld, cols <= src_ld, rows and pitches below 2^20, rows * dst_cols below 2^31");
  VITMI_REQUIRE(is_aligned(src, dtype_size(dtype)) && is_aligned(dst, dtype_size(dtype)), VITMI_E_ALIGN,
                "conv3s2_wcopy: misaligned pointer");
  const int64_t blocks = (rows * dst_cols + NT - 1) / NT;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == VITMI_BF16)
    hipLaunchKernelGGL((wcopy_kernel<bf16>), dim3((unsigned)blocks), dim3(NT), 0, s, (const bf16*)src, src_ld, (bf16*)dst, dst_ld,
                       rows, (int)cols, (int)dst_cols);
  else
    hipLaunchKernelGGL((wcopy_kernel<float>), dim3((unsigned)blocks), dim3(NT), 0, s, (const float*)src, src_ld, (float*)dst, dst_ld,
                       rows, (int)cols, (int)dst_cols);
  return vitmi_check_launch("conv3s2 wcopy_kernel");
}

extern "C" int vitmi_bn_act_supported(int dtype, int64_t M, int64_t C) {
  return dtype_ok(dtype) && C >= 8 && C % 8 == 0 && C < (1 << 20) && M >= 1 && M < (1ll << 31);
}

// the per-chunk partial rows: (mean, M2) in double forward, dbeta | dgamma in fp32 backward
extern "C" size_t vitmi_bn_act_workspace(int dtype, int64_t M, int64_t C) {
  if (!vitmi_bn_act_supported(dtype, M, C)) return 0;
  const Geo g = row_geometry(dtype, M, C);
  return round256((size_t)g.nch * 2 * (size_t)C * sizeof(double));
}

extern "C" int vitmi_bn_act_fwd(const void* y, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                int64_t* num_batches_tracked, float* stat, void* out, int dtype, int gelu, int training,
                                float momentum, float eps, int64_t M, int64_t C, void* workspace, size_t workspace_bytes,
                                void* stream) {
  if (int rc = check_bn("bn_act_fwd", dtype, M, C, training)) return rc;
  VITMI_REQUIRE(y && gamma && beta && stat && out, VITMI_E_BADARG, "bn_act_fwd: null pointer");
  VITMI_REQUIRE(training || (running_mean && running_var), VITMI_E_BADARG, "bn_act_fwd: eval mode needs the running buffers");
  VITMI_REQUIRE(is_aligned(y, 16) && is_aligned(out, 16) && is_aligned(stat, 16) && is_aligned(gamma, 16) &&
                    is_aligned(beta, 16) && is_aligned(running_mean, 4) && is_aligned(running_var, 4) &&
                    is_aligned(num_batches_tracked, 8),
                VITMI_E_ALIGN, "bn_act_fwd: y, out, stat, gamma and beta must be 16-B aligned");
  VITMI_REQUIRE(workspace && is_aligned(workspace, 16) && workspace_bytes >= vitmi_bn_act_workspace(dtype, M, C),
                VITMI_E_WORKSPACE, "bn_act_fwd: workspace missing, not 16-B aligned or smaller than vitmi_bn_act_workspace");
  const Geo g = row_geometry(dtype, M, C);
  const RowDims d = rows_of(g, C);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == VITMI_BF16)
    return bn_fwd<bf16>((const bf16*)y, gamma, beta, running_mean, running_var, num_batches_tracked, stat, (bf16*)out, gelu,
                        training, momentum, eps, g, d, (double*)workspace, s);
  return bn_fwd<float>((const float*)y, gamma, beta, running_mean, running_var, num_batches_tracked, stat, (float*)out, gelu,
                       training, momentum, eps, g, d, (double*)workspace, s);
}

extern "C" int vitmi_bn_act_bwd(const void* dout, const void* y, const float* stat, const float* gamma, const float* beta,
                                void* dy, float* dgamma, float* dbeta, int dtype, int gelu, int training, int64_t M, int64_t C,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_bn("bn_act_bwd", dtype, M, C, training)) return rc;
  VITMI_REQUIRE(dout && y && stat && gamma && beta && dy && dgamma && dbeta, VITMI_E_BADARG, "bn_act_bwd: null pointer");
  VITMI_REQUIRE(is_aligned(dout, 16) && is_aligned(y, 16) && is_aligned(dy, 16) && is_aligned(stat, 16) &&
                    is_aligned(gamma, 16) && is_aligned(beta, 16) && is_aligned(dgamma, 16) && is_aligned(dbeta, 16),
                VITMI_E_ALIGN, "bn_act_bwd: dout, y, dy, stat, gamma, beta, dgamma and dbeta must be 16-B aligned");
  VITMI_REQUIRE(workspace && is_aligned(workspace, 16) && workspace_bytes >= vitmi_bn_act_workspace(dtype, M, C),
                VITMI_E_WORKSPACE, "bn_act_bwd: workspace missing, not 16-B aligned or smaller than vitmi_bn_act_workspace");
  const Geo g = row_geometry(dtype, M, C);
  const RowDims d = rows_of(g, C);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* part = (float*)workspace;
  if (dtype == VITMI_BF16) {
    if (gelu)
      return bn_bwd<bf16, true>((const bf16*)dout, (const bf16*)y, stat, gamma, beta, (bf16*)dy, dgamma, dbeta, training, g, d,
                                part, s);
    return bn_bwd<bf16, false>((const bf16*)dout, (const bf16*)y, stat, gamma, beta, (bf16*)dy, dgamma, dbeta, training, g, d,
                               part, s);
  }
  if (gelu)
    return bn_bwd<float, true>((const float*)dout, (const float*)y, stat, gamma, beta, (float*)dy, dgamma, dbeta, training, g, d,
                               part, s);
  return bn_bwd<float, false>((const float*)dout, (const float*)y, stat, gamma, beta, (float*)dy, dgamma, dbeta, training, g, d,
                              part, s);
}
