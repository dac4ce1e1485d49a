// Materialised attention probabilities P[b,h,i,j] = softmax_j(scale * q_i . k_j) (fp32, [B, H, N, N]) for DINO's
// get_last_selfattention: the flash-style forwards (attention.hip, attention_f32.hip) never write P.
//
// qkv is the qkv Linear's output [B, N, 3, H, hd] exactly as vitmi_attn_fwd reads it (token stride 3 H hd).  One wave
// owns a block of 32 queries of one (image, head) and walks the keys in blocks of 32, twice:
//   pass 1: S = Q K^T on the matrix pipe, running row max and row sum (in natural units, the scale applied after the
//           product as DINO writes `(q @ k^T) * scale`)
//   pass 2: S again, P = exp(s - m) / l stored straight from the accumulator.
// S = Q K^T puts the key on the lane and the query rows in the accumulator registers (C layout: row = crow(r, hf),
// col = lane & 31), so each store instruction writes 32 consecutive keys of two query rows: 128-byte runs of dwords.
// Rows of P start only 4-byte aligned when N is odd, so every store is a dword; every offset into P is 64-bit (B H N^2
// exceeds 2^31 at real sizes).  The recompute is cheap next to the store (2 N^2 hd FLOPs against 4 N^2 bytes per
// (image, head)): the bf16 form is bound by HBM writes.  K fragments come straight from global memory (L2: the waves
// of one (image, head) read the same K), the next key block's fragments loaded while the current one is processed.
//   bf16: v_mfma_f32_32x32x16_bf16, lane (r, h) holds A[r][8h + j] / B[8h + j][r] (8 bf16 = one 16-byte load)
//   fp32: v_mfma_f32_32x32x2_f32, the contraction enumerated as d = 8t + 4hf + j in both operands (attention_f32.hip)
#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int WAVES = 4;                 // waves (query blocks of 32) per workgroup

__device__ __forceinline__ int crow(int r, int hf) { return (r & 3) + 8 * (r >> 2) + 4 * hf; }
__device__ __forceinline__ float exp_nat(float x) { return __builtin_amdgcn_exp2f(x * LOG2E); }

// operand fragments of one row (query or key) and the 32x32 product of two such sets
template <typename T, int HD> struct Frag;
template <int HD> struct Frag<bf16, HD> {
  static constexpr int NF = HD / 16;
  bf16x8 v[NF];
  __device__ __forceinline__ void load(const bf16* row, int hf) {
#pragma unroll
    for (int s = 0; s < NF; ++s) v[s] = *reinterpret_cast<const bf16x8*>(row + 16 * s + 8 * hf);
  }
};
template <int HD> struct Frag<float, HD> {
  static constexpr int NF = HD / 8;
  f32x4 v[NF];
  __device__ __forceinline__ void load(const float* row, int hf) {
#pragma unroll
    for (int t = 0; t < NF; ++t) v[t] = *reinterpret_cast<const f32x4*>(row + 8 * t + 4 * hf);
  }
};

template <int HD> __device__ __forceinline__ f32x16 qk(const Frag<bf16, HD>& q, const Frag<bf16, HD>& k) {
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
  for (int s = 0; s < Frag<bf16, HD>::NF; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(q.v[s], k.v[s], acc, 0, 0, 0);
  return acc;
}
template <int HD> __device__ __forceinline__ f32x16 qk(const Frag<float, HD>& q, const Frag<float, HD>& k) {
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
  for (int t = 0; t < Frag<float, HD>::NF; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(q.v[t][j], k.v[t][j], acc, 0, 0, 0);
  return acc;
}

// (m, l) of a row merged with another lane's: l = l_a e^(m_a - m) + l_b e^(m_b - m); an empty side (m = -inf) adds 0
__device__ __forceinline__ void merge_ml(float& m, float& l, float mo, float lo) {
  const float mx = fmaxf(m, mo);
  const float ea = m == -INFINITY ? 0.f : exp_nat(m - mx);
  const float eb = mo == -INFINITY ? 0.f : exp_nat(mo - mx);
  l = l * ea + lo * eb;
  m = mx;
}

// S = Q K^T for key blocks 0 .. 2 ceil(nkb / 2) - 1 (past the last block the key rows clamp to N - 1), body(s, block)
// after each.  K fragments ping-pong between two register sets, each loaded one block ahead: the wait for a block's
// fragments then leaves the previous block's stores in flight (stores count in vmcnt too, and a loop whose loads land in
// the registers the MFMAs just read waits for everything at its top).
template <typename T, int HD, typename Body>
__device__ __forceinline__ void walk_keys(const Frag<T, HD>& qf, const T* kb, int64_t ts, int64_t N, int hf, int l32,
                                          Body&& body) {
  const int64_t nkb = (N + 31) / 32;
  Frag<T, HD> ka, kc;
  ka.load(kb + min((int64_t)l32, N - 1) * ts, hf);
  __builtin_amdgcn_s_waitcnt(0x0F70);                  // vmcnt(0): the loop's first wait then matches every later one
  for (int64_t kbk = 0; kbk < nkb; kbk += 2) {
    kc.load(kb + min(kbk * 32 + 32 + l32, N - 1) * ts, hf);
    body(qk<HD>(qf, ka), kbk);
    ka.load(kb + min(kbk * 32 + 64 + l32, N - 1) * ts, hf);
    body(qk<HD>(qf, kc), kbk + 1);
  }
}

// P rows q0 .. q0 + 31 (pb = row q0), keys 0 .. N-1; RAGGED: the block holds rows past N (row index clamped to last)
template <typename T, int HD, bool RAGGED>
__device__ __forceinline__ void pass2(const Frag<T, HD>& qf, const T* kb, int64_t ts, float* pb, int64_t N, int64_t last,
                                      const float (&m)[16], const float (&l)[16], float scale, int hf, int l32) {
  int64_t roff[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = RAGGED ? min((int64_t)crow(r, hf), last) : crow(r, hf);
    roff[r] = row * N;
  }
  walk_keys<T, HD>(qf, kb, ts, N, hf, l32, [&](const f32x16& s, int64_t kbk) {
    const int64_t key = min(kbk * 32 + l32, N - 1);      // a block past the last one re-stores key N - 1
#pragma unroll
    for (int r = 0; r < 16; ++r) pb[roff[r] + key] = exp_nat(s[r] * scale - m[r]) * l[r];
  });
}

// grid-stride over work items (image-head, group of WAVES query blocks)
template <typename T, int HD>
__global__ __launch_bounds__(64 * WAVES) void attn_probs_kernel(const T* __restrict__ qkv, float* __restrict__ P, int64_t N,
                                                                int64_t H, int64_t groups, int64_t items, float scale) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hf = lane >> 5, l32 = lane & 31;
  const int64_t ts = 3 * H * HD;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t bh = item / groups, qblk = (item % groups) * WAVES + w;
    const int64_t q0 = qblk * 32;
    if (q0 >= N) continue;                              // wave-uniform: this wave's block lies past the last query
    const int64_t b = bh / H, h = bh % H;
    const T* qb = qkv + b * N * ts + h * HD;
    const T* kb = qb + H * HD;
    Frag<T, HD> qf;
    qf.load(qb + min(q0 + l32, N - 1) * ts, hf);        // rows past N: row N - 1 again

    // pass 1: lane-local running (max, sum) per accumulator row, over this lane's keys
    float m[16], l[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { m[r] = -INFINITY; l[r] = 0.f; }
    walk_keys<T, HD>(qf, kb, ts, N, hf, l32, [&](const f32x16& s, int64_t kbk) {
      if (kbk * 32 + l32 < N) {                         // keys past N (and a whole block past the last) count nothing
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          // one exp per score: e = e^-(|t - m|); the new max either rescales the sum or the new term
          const float t = s[r] * scale;
          const float e = exp_nat(fminf(t, m[r]) - fmaxf(t, m[r]));
          l[r] = t > m[r] ? l[r] * e + 1.f : l[r] + e;
          m[r] = fmaxf(m[r], t);
        }
      }
    });
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) merge_ml(m[r], l[r], __shfl_xor(m[r], o), __shfl_xor(l[r], o));
      l[r] = 1.f / l[r];
    }

    // pass 2: recompute and store.  Every lane stores every register: a lane past the last key or query (or in the padding
    // block of an odd block count) re-stores the element of key N-1 / query N-1, whose operands it loaded (clamped) and
    // whose value it computed bit for bit.  So each key block issues a fixed 16 stores and no branch.
    if (q0 + 32 <= N) pass2<T, HD, false>(qf, kb, ts, P + (bh * N + q0) * N, N, N - 1 - q0, m, l, scale, hf, l32);
    else pass2<T, HD, true>(qf, kb, ts, P + (bh * N + q0) * N, N, N - 1 - q0, m, l, scale, hf, l32);
  }
}

template <typename T, int HD>
int launch(const void* qkv, float* P, int64_t B, int64_t N, int64_t H, float scale, hipStream_t stream) {
  const int64_t groups = ((N + 31) / 32 + WAVES - 1) / WAVES;
  const int64_t items = B * H * groups;
  const int64_t grid = items < (1 << 20) ? items : (1 << 20);
  hipLaunchKernelGGL((attn_probs_kernel<T, HD>), dim3((unsigned)grid), dim3(64 * WAVES), 0, stream,
                     reinterpret_cast<const T*>(qkv), P, N, H, groups, items, scale);
  return vitmi_check_launch("attn_probs_kernel");
}

}  // namespace

extern "C" int vitmi_attn_probs(const void* qkv, float* P, int dtype, int64_t B, int64_t N, int64_t H, int64_t hd,
                                float scale, void* stream) {
  VITMI_REQUIRE(qkv && P && B > 0 && N > 0 && H > 0, VITMI_E_BADARG, "attn_probs: null pointer or empty shape");
  VITMI_REQUIRE(dtype == VITMI_BF16 || dtype == VITMI_F32, VITMI_E_DTYPE, "attn_probs: qkv must be bf16 or fp32");
  VITMI_REQUIRE(hd == 32 || hd == 64, VITMI_E_SHAPE, "attn_probs: head dim %lld not in {32, 64}", (long long)hd);
  VITMI_REQUIRE(is_aligned(qkv, 16), VITMI_E_ALIGN, "attn_probs: qkv must be 16-B aligned");
  VITMI_REQUIRE(is_aligned(P, 4), VITMI_E_ALIGN, "attn_probs: P must be 4-B aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == VITMI_BF16) return hd == 64 ? launch<bf16, 64>(qkv, P, B, N, H, scale, s) : launch<bf16, 32>(qkv, P, B, N, H, scale, s);
  return hd == 64 ? launch<float, 64>(qkv, P, B, N, H, scale, s) : launch<float, 32>(qkv, P, B, N, H, scale, s);
}
