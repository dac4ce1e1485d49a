// XCiT's cross-covariance attention (XCA, models/xcit.py:237-257 of the reference): attention over CHANNELS.  Per (image,
// head) pair, with Q, K, V [N, d] the head's slices of qkv [B, N, 3, H, d] (the layout vitmi_attn_fwd reads), tau the
// head's temperature:
//   r_q[i] = max(|Q[:, i]|_2, 1e-12), r_k likewise        G = Q^T K (d x d, the only reduction over N)
//   Gh[i][j] = G[i][j] / (r_q[i] r_k[j])                   A = softmax_j(tau Gh)        O[n][i] = sum_j A[i][j] V[n][j]
// and, for dO [B, N, H, d]:
//   dA = dO^T V       dV = dO A       dS = A o (dA - rowsum(A o dA))       dtau = sum_ij dS o Gh       dGh = tau dS
//   c[i] = sum_j dGh o Gh   e[j] = sum_i dGh o Gh   M = dGh / (r_q r_k)
//   dQ[n][i] = sum_j M[i][j] K[n][j] - Q[n][i] c[i] / r_q[i]^2      dK[n][j] = sum_i M[i][j] Q[n][i] - K[n][j] e[j] / r_k[j]^2
// The forward keeps stat [B, H, d+2, d] fp32 (rows 0..d-1 Gh, row d r_q, row d+1 r_k) and nothing of size N; the backward
// recomputes A from Gh and tau.
//
// One workgroup of four waves owns a pair (grid-stride over pairs); every kernel runs three stages.
//   stage 1  the reduction over tokens (Q^T K, or dO^T V).  Both operands are staged row-major, [token][channel], in LDS in
//            chunks of `ch` tokens (rows past N zero) and read back with ds_read_b64_tr_b16, which hands
//            v_mfma_f32_16x16x32_bf16 fragments whose contraction index runs along the image's ROWS: no transposed copy
//            exists anywhere.  Wave w takes the 32-token steps w, w+4, .. of each chunk and accumulates all (d/16)^2 tiles;
//            the squared norms are the diagonals of Q^T Q and K^T K, two more MFMAs per tile column on fragments already
//            in registers.  The four waves' tiles are then added in LDS in wave order (fixed order: bitwise repeatable).
//   stage 2  the d x d mathematics in fp32, four threads per row (norms, Gh, softmax, dS, c, e, M, dtau).  It leaves the
//            operands of stage 3 in LDS as bf16 images [channel][64] (columns past d zero): A in the forward; A^T, M and
//            M^T in the backward.  These are the op's only roundings besides the stores.
//   stage 3  the token-sized products, 16 tokens per wave step: the d x d image is the A operand (ds_read_b128 rows), the
//            token rows are the B operand, 16 bytes per lane straight from global memory (they are contiguous along the
//            contraction).  The accumulator then holds 4 consecutive channels of one token per lane: 8-byte stores.  The
//            normalisation terms Q c / r_q^2 and K e / r_k^2 are subtracted in fp32 before the store.
// Traffic: forward qkv once + O once.  Backward qkv once + dqkv once + dO once or twice: when N <= XCA_RESIDENT_N (256)
// stage 1 stages the pair's whole dO and V slices as ONE chunk and stage 3 takes its dO fragments from that LDS image
// (dO read once); a longer sequence streams 128-token chunks and stage 3 reads dO from global memory again.  LDS at
// N = 196, d = 48, backward: 2 x 224 x 96 B images + 10.4 KB fp32 + 3 x 6.9 KB bf16 images = 74 KB (two workgroups per
// CU); the largest, N = 256 at d = 64, is 127 KB.  No atomics: dtemp_part [B, H] is one store per pair.
//
// The fp32 form (T = float, the parity modes) is a plain VALU kernel with the same three stages and the same stage 2.
#include "common.h"

namespace {

constexpr int WAVES = 4, NT = 64 * WAVES;
constexpr int XCA_RESIDENT_N = 256;      // backward: dO and V stay in LDS between stage 1 and stage 3 up to this N
constexpr int XCA_STREAM_CH = 128;       // tokens per staged chunk otherwise
constexpr int XCA_MAX_LDS = 136 * 1024;  // raised once per kernel: covers the largest carve (bf16 backward, N = 256, d = 64: 126 KB)
constexpr int KP = 64;                   // contraction columns of the d x d bf16 images (zero past d)
constexpr int AP = KP * 2 + 16;          // their row pitch in bytes
constexpr float LOG2E = 1.4426950408889634f;
constexpr float NORM_EPS = 1e-12f;       // F.normalize's eps

__device__ __forceinline__ float exp_nat(float x) { return __builtin_amdgcn_exp2f(x * LOG2E); }
__device__ __forceinline__ float quad_sum(float v) { v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); return v; }
__device__ __forceinline__ float quad_max(float v) { v = fmaxf(v, __shfl_xor(v, 1)); return fmaxf(v, __shfl_xor(v, 2)); }
__device__ __forceinline__ bf16x8 zero8() {
  bf16x8 z;
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = (bf16)0.f;
  return z;
}

// row pitch (bytes) of a staged [token][d] bf16 image: 128-byte rows get 32 bytes of padding for the transposed reads
template <int HD> constexpr int tok_pitch() { return HD * 2 + ((HD * 2) % 128 == 0 ? 32 : 0); }
// row pitch (floats) of the fp32 d x d region: = 4 mod 32, so the four-threads-per-row walk of stage 2 is conflict-free
template <int HD> constexpr int r_pitch() { return HD + 4; }

// LDS carve (bytes) for chunk capacity ch tokens
template <typename T, int HD> struct Carve {
  static constexpr int TP = sizeof(T) == 2 ? tok_pitch<HD>() : HD * 4;     // fp32 form: plain [token][d] floats
  static constexpr int IMG = sizeof(T) == 2 ? HD * AP : HD * r_pitch<HD>() * 4;   // one d x d stage-3 image
  static constexpr int R = (HD + 2) * r_pitch<HD>() * 4;
  static constexpr int SMALL = 4 * 64 * 4;                // cq, ek, row sums, spare
  static __host__ __device__ int img_off(int ch) { return 2 * ch * TP; }
  static __host__ __device__ int r_off(int ch) { return img_off(ch) + 3 * IMG; }
  static __host__ __device__ int small_off(int ch) { return r_off(ch) + R; }
  static __host__ __device__ int total(int ch) { return small_off(ch) + SMALL; }
};

// ---------------------------------------------------------------------------------------------- stage 1, bf16 ---
// rows [n0, n0 + rows) of X and Y (token strides xs, ys) -> their images; rows up to rows_pad are zeroed.  Loads are
// unconditional (clamped row) and issued four pieces per operand ahead of their LDS writes.
template <int HD>
__device__ __forceinline__ void stage_pair(char* ix, char* iy, const bf16* X, int64_t xs, const bf16* Y, int64_t ys,
                                           int n0, int rows, int rows_pad, int tid) {
  constexpr int CPR = HD / 8, TP = tok_pitch<HD>(), NP = 4;
  const int total = rows_pad * CPR;
  for (int c0 = tid; c0 < total; c0 += NT * NP) {
    bf16x8 vx[NP], vy[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const int c = min(c0 + u * NT, total - 1), r = c / CPR, pc = c - r * CPR;
      const int64_t row = n0 + min(r, rows - 1);
      vx[u] = *reinterpret_cast<const bf16x8*>(X + row * xs + pc * 8);
      vy[u] = *reinterpret_cast<const bf16x8*>(Y + row * ys + pc * 8);
      if (r >= rows) { vx[u] = zero8(); vy[u] = zero8(); }
    }
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const int c = c0 + u * NT;
      if (c < total) {
        const int r = c / CPR, pc = c - r * CPR;
        *reinterpret_cast<bf16x8*>(ix + r * TP + pc * 16) = vx[u];
        *reinterpret_cast<bf16x8*>(iy + r * TP + pc * 16) = vy[u];
      }
    }
  }
}

// operand fragment whose contraction index runs along the ROWS of an image [k][c]: lane (g = lane >> 4, i = lane & 15)
// receives k = k0 + 8g .. +7 of column c0 + i (gemm_small.hip's tr_frag).  Needs every lane active.
__device__ __forceinline__ bf16x8 tr_frag(const char* img, int pitch, int k0, int c0, int lane) {
  const int g = lane >> 4, i = lane & 15;
  const char* p = img + (k0 + 8 * g + (i >> 2)) * pitch + (c0 + 4 * (i & 3)) * 2;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(LDS_PTR(bf16x4, p));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(LDS_PTR(bf16x4, p + 4 * pitch));
  bf16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}

template <int HD, bool NORMS> struct Acc {
  static constexpr int T = HD / 16;
  f32x4 g[T][T], nx[T], ny[T];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int a = 0; a < T; ++a) {
#pragma unroll
      for (int r = 0; r < 4; ++r) nx[a][r] = ny[a][r] = 0.f;
#pragma unroll
      for (int b = 0; b < T; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) g[a][b][r] = 0.f;
    }
  }
  // this wave's 32-token steps of a staged chunk: g += X^T Y (and the diagonals' tiles of X^T X, Y^T Y)
  __device__ __forceinline__ void chunk(const char* ix, const char* iy, int rows_pad, int w, int lane) {
    constexpr int TP = tok_pitch<HD>();
    for (int ks = w; ks < rows_pad / 32; ks += WAVES) {
      bf16x8 xf[T], yf[T];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        xf[t] = tr_frag(ix, TP, 32 * ks, 16 * t, lane);
        yf[t] = tr_frag(iy, TP, 32 * ks, 16 * t, lane);
      }
#pragma unroll
      for (int a = 0; a < T; ++a) {
#pragma unroll
        for (int b = 0; b < T; ++b) g[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[a], yf[b], g[a][b], 0, 0, 0);
        if (NORMS) {
          nx[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[a], xf[a], nx[a], 0, 0, 0);
          ny[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[a], yf[a], ny[a], 0, 0, 0);
        }
      }
    }
  }
  // the four waves' sums into R [d + 2][r_pitch] in wave order (C layout: row 4g + r, column lane & 15)
  __device__ __forceinline__ void reduce(float* R, int w, int lane) {
    constexpr int P = r_pitch<HD>();
    const int g4 = 4 * (lane >> 4), c = lane & 15;
    for (int ww = 0; ww < WAVES; ++ww) {
      if (w == ww) {
#pragma unroll
        for (int a = 0; a < T; ++a) {
#pragma unroll
          for (int b = 0; b < T; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float* p = R + (16 * a + g4 + r) * P + 16 * b + c;
              *p = (ww ? *p : 0.f) + g[a][b][r];
            }
          if (NORMS && (c >> 2) == (lane >> 4)) {      // the lane that holds the diagonal element of column c
            float* px = R + HD * P + 16 * a + c;
            float* py = px + P;
            float dx = 0.f, dy = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if ((c & 3) == r) { dx = nx[a][r]; dy = ny[a][r]; }
            *px = (ww ? *px : 0.f) + dx;
            *py = (ww ? *py : 0.f) + dy;
          }
        }
      }
      __syncthreads();
    }
  }
};

// ---------------------------------------------------------------------------------------------- stage 1, fp32 ---
// G += X^T Y over tokens, 32 staged at a time; thread t owns elements t, t + 256, .. of the d x d matrix and, for
// t < 2 d, one squared norm.  Chunk sums are formed first and then added to the running sums.
template <int HD, bool NORMS>
__device__ __forceinline__ void reduce_f32(float* xs_, float* ys_, float* R, const float* X, int64_t xs, const float* Y,
                                           int64_t ys, int N, int tid) {
  constexpr int E = HD * HD / NT, P = r_pitch<HD>(), CH = 32;
  float acc[E], nrm = 0.f;
  int io[E], jo[E];
#pragma unroll
  for (int u = 0; u < E; ++u) {
    const int e = tid + u * NT;
    io[u] = e / HD;
    jo[u] = e - io[u] * HD;
    acc[u] = 0.f;
  }
  for (int n0 = 0; n0 < N; n0 += CH) {
    const int rows = min(CH, N - n0);
    __syncthreads();
    for (int c = tid; c < CH * HD / 4; c += NT) {
      const int r = c / (HD / 4), pc = c - r * (HD / 4);
      const int64_t row = n0 + min(r, rows - 1);
      f32x4 vx = *reinterpret_cast<const f32x4*>(X + row * xs + pc * 4);
      f32x4 vy = *reinterpret_cast<const f32x4*>(Y + row * ys + pc * 4);
      if (r >= rows) { vx = f32x4{0.f, 0.f, 0.f, 0.f}; vy = vx; }
      *reinterpret_cast<f32x4*>(xs_ + r * HD + pc * 4) = vx;
      *reinterpret_cast<f32x4*>(ys_ + r * HD + pc * 4) = vy;
    }
    __syncthreads();
    float part[E];
#pragma unroll
    for (int u = 0; u < E; ++u) part[u] = 0.f;
#pragma unroll 2
    for (int n = 0; n < CH; ++n)
#pragma unroll
      for (int u = 0; u < E; ++u) part[u] = fmaf(xs_[n * HD + io[u]], ys_[n * HD + jo[u]], part[u]);
#pragma unroll
    for (int u = 0; u < E; ++u) acc[u] += part[u];
    if (NORMS && tid < 2 * HD) {
      const float* src = tid < HD ? xs_ + tid : ys_ + (tid - HD);
      float s = 0.f;
#pragma unroll 4
      for (int n = 0; n < CH; ++n) s = fmaf(src[n * HD], src[n * HD], s);
      nrm += s;
    }
  }
#pragma unroll
  for (int u = 0; u < E; ++u) R[io[u] * P + jo[u]] = acc[u];
  if (NORMS && tid < 2 * HD) R[(HD + (tid >= HD)) * P + (tid < HD ? tid : tid - HD)] = nrm;
  __syncthreads();
}

// ----------------------------------------------------------------------------------------------------- stage 2 ---
// element (row, col) of a d x d stage-3 image: bf16 images have 64 columns (zero past d), fp32 ones r_pitch
template <typename IT, int HD> __device__ __forceinline__ IT* img_at(char* img, int row, int col) {
  return sizeof(IT) == 2 ? reinterpret_cast<IT*>(img + row * AP) + col
                         : reinterpret_cast<IT*>(img) + row * r_pitch<HD>() + col;
}
template <typename IT, int HD> __device__ __forceinline__ void zero_pad(char* img, int i, int q) {
  if (sizeof(IT) == 2)
    for (int j = HD + q; j < KP; j += 4) *img_at<IT, HD>(img, i, j) = (IT)0.f;
}

// forward: R (raw G, squared norms) -> stat (global), A image.  Thread (i = tid >> 2, q = tid & 3) owns columns q + 4 jj
// of row i; rows past d compute on row d - 1 and store nothing.
template <typename IT, int HD>
__device__ __forceinline__ void dd_fwd(const float* R, float* stat, float tau, char* aimg, int tid) {
  constexpr int P = r_pitch<HD>(), J = HD / 4;
  const int i = min(tid >> 2, HD - 1), q = tid & 3;
  const bool live = (tid >> 2) < HD;
  const float rq = fmaxf(sqrtf(R[HD * P + i]), NORM_EPS);
  float s[J], m = -INFINITY;
#pragma unroll
  for (int jj = 0; jj < J; ++jj) {
    const int j = q + 4 * jj;
    const float rk = fmaxf(sqrtf(R[(HD + 1) * P + j]), NORM_EPS);
    const float gh = R[i * P + j] / (rq * rk);
    if (live) stat[i * HD + j] = gh;
    s[jj] = tau * gh;
    m = fmaxf(m, s[jj]);
  }
  m = quad_max(m);
  float l = 0.f;
#pragma unroll
  for (int jj = 0; jj < J; ++jj) { s[jj] = exp_nat(s[jj] - m); l += s[jj]; }
  l = 1.f / quad_sum(l);
  if (live) {
#pragma unroll
    for (int jj = 0; jj < J; ++jj) *img_at<IT, HD>(aimg, i, q + 4 * jj) = (IT)(s[jj] * l);
    zero_pad<IT, HD>(aimg, i, q);
    if (q == 0) stat[HD * HD + i] = rq;
  }
  if (tid < HD) stat[(HD + 1) * HD + tid] = fmaxf(sqrtf(R[(HD + 1) * P + tid]), NORM_EPS);
}

// backward: R (dA) and stat -> images A^T, M, M^T, cq[i] = c[i] / r_q[i]^2, ek[j] = e[j] / r_k[j]^2, dtemp_part
template <typename IT, int HD>
__device__ __forceinline__ void dd_bwd(float* R, const float* stat, float tau, char* atimg, char* mimg, char* mtimg,
                                       float* cq, float* ek, float* rowsum, float* dtemp, int tid) {
  constexpr int P = r_pitch<HD>(), J = HD / 4;
  const int i = min(tid >> 2, HD - 1), q = tid & 3;
  const bool live = (tid >> 2) < HD;
  const float rq = stat[HD * HD + i];
  float gh[J], a[J], m = -INFINITY;
#pragma unroll
  for (int jj = 0; jj < J; ++jj) {
    gh[jj] = stat[i * HD + q + 4 * jj];
    m = fmaxf(m, tau * gh[jj]);
  }
  m = quad_max(m);
  float l = 0.f, dot = 0.f;
#pragma unroll
  for (int jj = 0; jj < J; ++jj) { a[jj] = exp_nat(tau * gh[jj] - m); l += a[jj]; }
  l = 1.f / quad_sum(l);
#pragma unroll
  for (int jj = 0; jj < J; ++jj) { a[jj] *= l; dot += a[jj] * R[i * P + q + 4 * jj]; }
  dot = quad_sum(dot);
  float dt = 0.f, c = 0.f, mv[J];
#pragma unroll
  for (int jj = 0; jj < J; ++jj) {
    const int j = q + 4 * jj;
    const float ds = a[jj] * (R[i * P + j] - dot);
    const float dg = tau * ds;
    dt += ds * gh[jj];
    c += dg * gh[jj];
    mv[jj] = dg / (rq * stat[(HD + 1) * HD + j]);
    if (live) R[i * P + j] = dg * gh[jj];              // for the column sums e[j]; each element is its owner's alone
  }
  dt = quad_sum(dt);
  c = quad_sum(c);
  if (live) {
#pragma unroll
    for (int jj = 0; jj < J; ++jj) {
      const int j = q + 4 * jj;
      *img_at<IT, HD>(atimg, j, i) = (IT)a[jj];
      *img_at<IT, HD>(mimg, i, j) = (IT)mv[jj];
      *img_at<IT, HD>(mtimg, j, i) = (IT)mv[jj];
    }
    zero_pad<IT, HD>(atimg, i, q);
    zero_pad<IT, HD>(mimg, i, q);
    zero_pad<IT, HD>(mtimg, i, q);
    if (q == 0) { cq[i] = c / (rq * rq); rowsum[i] = dt; }
  }
  __syncthreads();
  if (tid < HD) {
    float e = 0.f;
    for (int r = 0; r < HD; ++r) e += R[r * P + tid];
    const float rk = stat[(HD + 1) * HD + tid];
    ek[tid] = e / (rk * rk);
  }
  if (tid == 0) {
    float t = 0.f;
    for (int r = 0; r < HD; ++r) t += rowsum[r];
    *dtemp = t;
  }
}

// ----------------------------------------------------------------------------------------------- stage 3, bf16 ---
// the 8 contraction elements 32 s + 8 g .. of token row `row` (clamped by the caller); zero past d.  LDS selects an image
// row (pitch bytes in `stride`) instead of a global row (stride in elements)
template <int HD>
__device__ __forceinline__ bf16x8 tok_frag(const bf16* X, int64_t stride, int64_t row, int k) {
  bf16x8 v = *reinterpret_cast<const bf16x8*>(X + row * stride + (k < HD ? k : 0));
  if (k >= HD) v = zero8();
  return v;
}
template <int HD>
__device__ __forceinline__ f32x4 dd_times_tok(const char* img, int t, const bf16x8 (&xf)[(HD + 31) / 32], int lane) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < (HD + 31) / 32; ++s) {
    const bf16x8 af = *reinterpret_cast<const bf16x8*>(img + (16 * t + (lane & 15)) * AP + (32 * s + 8 * (lane >> 4)) * 2);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, xf[s], acc, 0, 0, 0);
  }
  return acc;
}
__device__ __forceinline__ void store_bf16x4(bf16* p, const f32x4& v) {
  bf16x4 r = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
  *reinterpret_cast<bf16x4*>(p) = r;
}

// ------------------------------------------------------------------------------------------------- the kernels ---
template <int HD>
__global__ __launch_bounds__(NT) void xca_fwd_bf16(const bf16* __restrict__ qkv, const float* __restrict__ temp,
                                                   bf16* __restrict__ out, float* __restrict__ stat, int64_t pairs, int N,
                                                   int H, int ch) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  using CV = Carve<bf16, HD>;
  constexpr int T = HD / 16, KS = (HD + 31) / 32, TP = tok_pitch<HD>();
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
  char* iq = lds;
  char* ik = lds + ch * TP;
  char* aimg = lds + CV::img_off(ch);
  float* R = reinterpret_cast<float*>(lds + CV::r_off(ch));
  const int64_t ts = 3 * (int64_t)H * HD, os = (int64_t)H * HD;
  for (int64_t pair = blockIdx.x; pair < pairs; pair += gridDim.x) {
    const int64_t b = pair / H, h = pair - b * H;
    const bf16* Q = qkv + b * N * ts + h * HD;
    const bf16* K = Q + os;
    const bf16* V = K + os;
    Acc<HD, true> acc;
    acc.clear();
    for (int n0 = 0; n0 < N; n0 += ch) {
      const int rows = min(ch, N - n0), rows_pad = (rows + 31) & ~31;
      __syncthreads();
      stage_pair<HD>(iq, ik, Q, ts, K, ts, n0, rows, rows_pad, tid);
      __syncthreads();
      acc.chunk(iq, ik, rows_pad, w, lane);
    }
    acc.reduce(R, w, lane);
    dd_fwd<bf16, HD>(R, stat + pair * (HD + 2) * HD, temp[h], aimg, tid);
    __syncthreads();
    bf16* O = out + b * N * os + h * HD;
    for (int n0 = 16 * w; n0 < N; n0 += 16 * WAVES) {
      const int n = n0 + (lane & 15);
      const int64_t nc = min(n, N - 1);
      bf16x8 vf[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) vf[s] = tok_frag<HD>(V, ts, nc, 32 * s + 8 * g);
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const f32x4 o = dd_times_tok<HD>(aimg, t, vf, lane);
        if (n < N) store_bf16x4(O + n * os + 16 * t + 4 * g, o);
      }
    }
  }
}

template <int HD>
__global__ __launch_bounds__(NT) void xca_bwd_bf16(const bf16* __restrict__ qkv, const bf16* __restrict__ dout,
                                                   const float* __restrict__ temp, const float* __restrict__ stat,
                                                   bf16* __restrict__ dqkv, float* __restrict__ dtemp_part, int64_t pairs,
                                                   int N, int H, int ch) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  using CV = Carve<bf16, HD>;
  constexpr int T = HD / 16, KS = (HD + 31) / 32, TP = tok_pitch<HD>();
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
  char* ido = lds;
  char* iv = lds + ch * TP;
  char* atimg = lds + CV::img_off(ch);
  char* mimg = atimg + CV::IMG;
  char* mtimg = mimg + CV::IMG;
  float* R = reinterpret_cast<float*>(lds + CV::r_off(ch));
  float* cq = reinterpret_cast<float*>(lds + CV::small_off(ch));
  float* ek = cq + 64;
  float* rowsum = ek + 64;
  const int64_t ts = 3 * (int64_t)H * HD, os = (int64_t)H * HD;
  const bool resident = N <= ch;                     // one chunk: the dO image outlives stage 1
  for (int64_t pair = blockIdx.x; pair < pairs; pair += gridDim.x) {
    const int64_t b = pair / H, h = pair - b * H;
    const bf16* Q = qkv + b * N * ts + h * HD;
    const bf16* K = Q + os;
    const bf16* V = K + os;
    const bf16* dO = dout + b * N * os + h * HD;
    Acc<HD, false> acc;
    acc.clear();
    for (int n0 = 0; n0 < N; n0 += ch) {
      const int rows = min(ch, N - n0), rows_pad = (rows + 31) & ~31;
      __syncthreads();
      stage_pair<HD>(ido, iv, dO, os, V, ts, n0, rows, rows_pad, tid);
      __syncthreads();
      acc.chunk(ido, iv, rows_pad, w, lane);
    }
    acc.reduce(R, w, lane);
    dd_bwd<bf16, HD>(R, stat + pair * (HD + 2) * HD, temp[h], atimg, mimg, mtimg, cq, ek, rowsum, dtemp_part + pair, tid);
    __syncthreads();
    bf16* dQ = dqkv + b * N * ts + h * HD;
    bf16* dK = dQ + os;
    bf16* dV = dK + os;
    for (int n0 = 16 * w; n0 < N; n0 += 16 * WAVES) {
      const int n = n0 + (lane & 15);
      const int64_t nc = min(n, N - 1);
      bf16x8 qf[KS], kf[KS], df[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int k = 32 * s + 8 * g;
        qf[s] = tok_frag<HD>(Q, ts, nc, k);
        kf[s] = tok_frag<HD>(K, ts, nc, k);
        if (resident) {
          df[s] = *reinterpret_cast<const bf16x8*>(ido + nc * TP + (k < HD ? k : 0) * 2);
          if (k >= HD) df[s] = zero8();
        } else {
          df[s] = tok_frag<HD>(dO, os, nc, k);
        }
      }
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const int c0 = 16 * t + 4 * g;
        const bf16x4 qs = *reinterpret_cast<const bf16x4*>(Q + nc * ts + c0);
        const bf16x4 ks = *reinterpret_cast<const bf16x4*>(K + nc * ts + c0);
        const f32x4 dv = dd_times_tok<HD>(atimg, t, df, lane);
        f32x4 dq = dd_times_tok<HD>(mimg, t, kf, lane);
        f32x4 dk = dd_times_tok<HD>(mtimg, t, qf, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          dq[r] -= (float)qs[r] * cq[c0 + r];
          dk[r] -= (float)ks[r] * ek[c0 + r];
        }
        if (n < N) {
          store_bf16x4(dQ + n * ts + c0, dq);
          store_bf16x4(dK + n * ts + c0, dk);
          store_bf16x4(dV + n * ts + c0, dv);
        }
      }
    }
  }
}

// fp32 stage 3: out[n][c] = sum_k img[c][k] X[n][k] - S[n][c] sub[c], one (token, channel) per thread step
template <int HD>
__device__ __forceinline__ void f32_product(const char* img, const float* X, int64_t xs, const float* S, int64_t ss,
                                            const float* sub, float* out, int64_t os, int N, int tid) {
  constexpr int P = r_pitch<HD>();
  const float* im = reinterpret_cast<const float*>(img);
  for (int e = tid; e < N * HD; e += NT) {
    const int n = e / HD, c = e - n * HD;
    const float* x = X + n * xs;
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < HD; ++k) s = fmaf(im[c * P + k], x[k], s);
    if (S) s -= S[n * ss + c] * sub[c];
    out[n * os + c] = s;
  }
}

template <int HD>
__global__ __launch_bounds__(NT) void xca_fwd_f32(const float* __restrict__ qkv, const float* __restrict__ temp,
                                                  float* __restrict__ out, float* __restrict__ stat, int64_t pairs, int N,
                                                  int H, int ch) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  using CV = Carve<float, HD>;
  const int tid = threadIdx.x;
  float* xs_ = reinterpret_cast<float*>(lds);
  float* ys_ = xs_ + ch * HD;
  char* aimg = lds + CV::img_off(ch);
  float* R = reinterpret_cast<float*>(lds + CV::r_off(ch));
  const int64_t ts = 3 * (int64_t)H * HD, os = (int64_t)H * HD;
  for (int64_t pair = blockIdx.x; pair < pairs; pair += gridDim.x) {
    const int64_t b = pair / H, h = pair - b * H;
    const float* Q = qkv + b * N * ts + h * HD;
    reduce_f32<HD, true>(xs_, ys_, R, Q, ts, Q + os, ts, N, tid);
    dd_fwd<float, HD>(R, stat + pair * (HD + 2) * HD, temp[h], aimg, tid);
    __syncthreads();
    f32_product<HD>(aimg, Q + 2 * os, ts, nullptr, 0, nullptr, out + b * N * os + h * HD, os, N, tid);
    __syncthreads();
  }
}

template <int HD>
__global__ __launch_bounds__(NT) void xca_bwd_f32(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                  const float* __restrict__ temp, const float* __restrict__ stat,
                                                  float* __restrict__ dqkv, float* __restrict__ dtemp_part, int64_t pairs,
                                                  int N, int H, int ch) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  using CV = Carve<float, HD>;
  const int tid = threadIdx.x;
  float* xs_ = reinterpret_cast<float*>(lds);
  float* ys_ = xs_ + ch * HD;
  char* atimg = lds + CV::img_off(ch);
  char* mimg = atimg + CV::IMG;
  char* mtimg = mimg + CV::IMG;
  float* R = reinterpret_cast<float*>(lds + CV::r_off(ch));
  float* cq = reinterpret_cast<float*>(lds + CV::small_off(ch));
  float* ek = cq + 64;
  float* rowsum = ek + 64;
  const int64_t ts = 3 * (int64_t)H * HD, os = (int64_t)H * HD;
  for (int64_t pair = blockIdx.x; pair < pairs; pair += gridDim.x) {
    const int64_t b = pair / H, h = pair - b * H;
    const float* Q = qkv + b * N * ts + h * HD;
    const float* K = Q + os;
    const float* dO = dout + b * N * os + h * HD;
    float* dQ = dqkv + b * N * ts + h * HD;
    reduce_f32<HD, false>(xs_, ys_, R, dO, os, K + os, ts, N, tid);
    dd_bwd<float, HD>(R, stat + pair * (HD + 2) * HD, temp[h], atimg, mimg, mtimg, cq, ek, rowsum, dtemp_part + pair, tid);
    __syncthreads();
    f32_product<HD>(atimg, dO, os, nullptr, 0, nullptr, dQ + 2 * os, ts, N, tid);
    f32_product<HD>(mimg, K, ts, Q, ts, cq, dQ, ts, N, tid);
    f32_product<HD>(mtimg, Q, ts, K, ts, ek, dQ + os, ts, N, tid);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------- dispatch ---
int chunk_tokens(int dtype, int64_t N, bool bwd) {
  if (dtype == VITMI_F32) return 32;
  const int n32 = (int)((N + 31) / 32 * 32);
  if (bwd) return N <= XCA_RESIDENT_N ? n32 : XCA_STREAM_CH;
  return n32 < XCA_STREAM_CH ? n32 : XCA_STREAM_CH;
}

template <typename Kern, typename... Args>
int launch(Kern kern, const char* who, int lds_bytes, int64_t pairs, hipStream_t stream, Args... args) {
  if (lds_bytes > 64 * 1024)
    if (int rc = vitmi_raise_dynamic_lds(reinterpret_cast<const void*>(kern), XCA_MAX_LDS, who)) return rc;
  const int64_t grid = pairs < (1 << 20) ? pairs : (1 << 20);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(NT), lds_bytes, stream, args...);
  return vitmi_check_launch(who);
}

int check_shape(const char* who, int dtype, int64_t B, int64_t N, int64_t H, int64_t hd) {
  VITMI_REQUIRE(dtype == VITMI_BF16 || dtype == VITMI_F32, VITMI_E_DTYPE, "%s: qkv must be bf16 or fp32", who);
  VITMI_REQUIRE(hd == 32 || hd == 48 || hd == 64, VITMI_E_SHAPE, "%s: head dim %lld not in {32, 48, 64}", who, (long long)hd);
  VITMI_REQUIRE(B >= 1 && H >= 1 && N >= 1 && N < (1 << 24) && H < (1 << 20), VITMI_E_SHAPE,
                "%s: B = %lld, H = %lld, N = %lld: every extent must be at least 1 (N < 2^24, H < 2^20)", who, (long long)B,
                (long long)H, (long long)N);
  return 0;
}

template <int HD>
int fwd(const void* qkv, const float* temp, void* out, float* stat, int dtype, int64_t B, int64_t N, int64_t H, hipStream_t s) {
  const int ch = chunk_tokens(dtype, N, false);
  if (dtype == VITMI_BF16)
    return launch(xca_fwd_bf16<HD>, "xca_fwd", Carve<bf16, HD>::total(ch), B * H, s, (const bf16*)qkv, temp, (bf16*)out, stat,
                  B * H, (int)N, (int)H, ch);
  return launch(xca_fwd_f32<HD>, "xca_fwd", Carve<float, HD>::total(ch), B * H, s, (const float*)qkv, temp, (float*)out, stat,
                B * H, (int)N, (int)H, ch);
}

template <int HD>
int bwd(const void* qkv, const void* dout, const float* temp, const float* stat, void* dqkv, float* dtemp_part, int dtype,
        int64_t B, int64_t N, int64_t H, hipStream_t s) {
  const int ch = chunk_tokens(dtype, N, true);
  if (dtype == VITMI_BF16)
    return launch(xca_bwd_bf16<HD>, "xca_bwd", Carve<bf16, HD>::total(ch), B * H, s, (const bf16*)qkv, (const bf16*)dout, temp,
                  stat, (bf16*)dqkv, dtemp_part, B * H, (int)N, (int)H, ch);
  return launch(xca_bwd_f32<HD>, "xca_bwd", Carve<float, HD>::total(ch), B * H, s, (const float*)qkv, (const float*)dout, temp,
                stat, (float*)dqkv, dtemp_part, B * H, (int)N, (int)H, ch);
}

}  // namespace

extern "C" int vitmi_xca_supported(int dtype, int64_t H, int64_t N, int64_t hd) {
  return (dtype == VITMI_BF16 || dtype == VITMI_F32) && (hd == 32 || hd == 48 || hd == 64) && H >= 1 && H < (1 << 20) &&
         N >= 1 && N < (1 << 24);
}

extern "C" size_t vitmi_xca_workspace(int64_t, int64_t, int64_t, int64_t) { return 0; }      // everything lives in LDS

extern "C" int vitmi_xca_fwd(const void* qkv, const float* temperature, void* out, float* stat, int dtype, int64_t B,
                             int64_t N, int64_t H, int64_t hd, void*, size_t, void* stream) {
  if (int rc = check_shape("xca_fwd", dtype, B, N, H, hd)) return rc;
  VITMI_REQUIRE(qkv && temperature && out && stat, VITMI_E_BADARG, "xca_fwd: null pointer");
  VITMI_REQUIRE(is_aligned(qkv, 16) && is_aligned(out, 16) && is_aligned(stat, 16) && is_aligned(temperature, 4), VITMI_E_ALIGN,
                "xca_fwd: qkv, out and stat must be 16-B aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hd == 32) return fwd<32>(qkv, temperature, out, stat, dtype, B, N, H, s);
  if (hd == 48) return fwd<48>(qkv, temperature, out, stat, dtype, B, N, H, s);
  return fwd<64>(qkv, temperature, out, stat, dtype, B, N, H, s);
}

extern "C" int vitmi_xca_bwd(const void* qkv, const void* dout, const float* temperature, const float* stat, void* dqkv,
                             float* dtemp_part, int dtype, int64_t B, int64_t N, int64_t H, int64_t hd, void*, size_t,
                             void* stream) {
  if (int rc = check_shape("xca_bwd", dtype, B, N, H, hd)) return rc;
  VITMI_REQUIRE(qkv && dout && temperature && stat && dqkv && dtemp_part, VITMI_E_BADARG, "xca_bwd: null pointer");
  VITMI_REQUIRE(is_aligned(qkv, 16) && is_aligned(dout, 16) && is_aligned(dqkv, 16) && is_aligned(stat, 16) &&
                    is_aligned(temperature, 4) && is_aligned(dtemp_part, 4),
                VITMI_E_ALIGN, "xca_bwd: qkv, dout, dqkv and stat must be 16-B aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hd == 32) return bwd<32>(qkv, dout, temperature, stat, dqkv, dtemp_part, dtype, B, N, H, s);
  if (hd == 48) return bwd<48>(qkv, dout, temperature, stat, dqkv, dtemp_part, dtype, B, N, H, s);
  return bwd<64>(qkv, dout, temperature, stat, dqkv, dtemp_part, dtype, B, N, H, s);
}
