// Device-side input pipeline with the reference's resize (utils_datasets.py:553-582 when the stored image size differs
// from the training size):  Resize(S, BICUBIC) -> RandomCrop(S, padding, fill=128) -> RandomHorizontalFlip -> ToTensor
// -> Normalize, on uint8 NHWC batches.  The resize is PIL's ImagingResample for 8-bit images, bit-exact: the
// fixed-point coefficient tables (22 fractional bits, built in double on the host: vit_torch_amd/resize.py) are
// INPUTS, the horizontal pass runs first over every source row the output needs and rounds to uint8, the vertical pass
// follows; each value is clamp((2^21 + sum src * k) >> 22, 0, 255) in int32.
//
// One workgroup = one image x one band of BR output rows.  It stages into LDS the source rows the band needs (one
// contiguous byte range of the NHWC image), the coefficient tables and a C x 256 lookup of the normalised values
// (the same expression as image_ingest: ((float)v / 255 - mean) / std), runs the horizontal pass into LDS as uint8
// (planar [c][row][Wr]), then the vertical pass + crop + flip + normalize from LDS, and stores 16 B per lane.  The
// resized image never reaches HBM: per image the kernel reads H*W*C bytes (plus the halo rows of neighbouring bands,
// from L2) and writes the output once.
//
// Table layout (int32, one per axis, n = output size of the axis, T = taps): start[n], count[n], k[T][n]
// (k[t][o] = 0 for t >= count[o]).
#include "common.h"

namespace {

constexpr int kTapLimit = 32;       // longest coefficient row a table may have (PIL: 2*ceil(2*max(in/out, 1)) + 1)
constexpr int kMaxLds = 64 * 1024;  // dynamic LDS one workgroup may ask for

__host__ __device__ inline int align16(int n) { return (n + 15) & ~15; }

struct ResizeGeom {
  int H, W, C, Hr, Wr, S, pad, fill;
  int ytaps, xtaps;
  int BR;        // output rows per band
  int rows_cap;  // most source rows one band can need
};

struct LdsLayout {
  int lut, xtab, ytab, src, mid, total;
};

__host__ __device__ inline LdsLayout lds_layout(const ResizeGeom& g) {
  LdsLayout L;
  L.lut = 0;
  L.xtab = L.lut + align16(g.C * 256 * 4);
  L.ytab = L.xtab + align16((2 + g.xtaps) * g.Wr * 4);
  L.src = L.ytab + align16((2 + g.ytaps) * g.BR * 4);
  L.mid = L.src + align16(g.rows_cap * g.W * g.C);
  L.total = L.mid + align16(g.C * g.rows_cap * g.Wr);
  return L;
}

// What a workgroup holds after resize_stage: the LDS views and the band's row windows.
struct Band {
  const float* lut;
  const int32_t* xs;   // xtab in LDS: start[Wr], count[Wr], k[T][Wr]
  const int32_t* ys;   // the band's y-table rows: start[BR], count[BR], k[T][BR]
  const uint8_t* mid;  // horizontal pass output, planar [C][nrows][Wr]
  int ry_lo, ry_hi;    // resized rows [ry_lo, ry_hi) the band reads
  int r0, nrows;       // source rows [r0, r0 + nrows) held in LDS
  int dy, dx;          // crop offset minus pad, per axis
  bool fl;
};

// Stage + horizontal pass for output rows [y0, y1) of image b.  Ends with a workgroup barrier.
__device__ Band resize_stage(uint8_t* lds, const ResizeGeom& g, const uint8_t* __restrict__ src,
                             const int32_t* __restrict__ ytab, const int32_t* __restrict__ xtab,
                             const int32_t* __restrict__ oy, const int32_t* __restrict__ ox,
                             const uint8_t* __restrict__ flip, const float* __restrict__ mean,
                             const float* __restrict__ stdv, int64_t b, int y0, int y1) {
  const LdsLayout L = lds_layout(g);
  const int tid = threadIdx.x, nt = blockDim.x;
  Band bd;
  bd.dy = (oy ? oy[b] : g.pad) - g.pad;
  bd.dx = (ox ? ox[b] : g.pad) - g.pad;
  bd.fl = flip && flip[b];
  bd.ry_lo = max(0, y0 + bd.dy);
  bd.ry_hi = min(g.Hr, y1 + bd.dy);
  bd.r0 = 0;
  bd.nrows = 0;
  if (bd.ry_lo < bd.ry_hi) {
    // tables are monotone (PIL): the first row's start and the last row's end bound every tap of the band
    const int last = bd.ry_hi - 1;
    const int r0 = min(max(ytab[bd.ry_lo], 0), g.H);
    const int r1 = min(min(ytab[last] + ytab[g.Hr + last], g.H), r0 + g.rows_cap);
    bd.r0 = r0;
    bd.nrows = max(r1 - r0, 0);
  }

  float* lut = reinterpret_cast<float*>(lds + L.lut);
  int32_t* xs = reinterpret_cast<int32_t*>(lds + L.xtab);
  int32_t* ys = reinterpret_cast<int32_t*>(lds + L.ytab);
  uint8_t* sl = lds + L.src;
  uint8_t* mid = lds + L.mid;

  for (int i = tid; i < g.C * 256; i += nt) {
    const int c = i >> 8, v = i & 255;
    const float mu = mean ? mean[c] : 0.f, sd = stdv ? stdv[c] : 1.f;
    lut[i] = ((float)v / 255.f - mu) / sd;
  }
  for (int i = tid; i < (2 + g.xtaps) * g.Wr; i += nt) xs[i] = xtab[i];
  const int nb = bd.ry_hi - bd.ry_lo;
  for (int i = tid; i < (2 + g.ytaps) * nb; i += nt) {
    const int t = i / nb, r = i - t * nb;
    ys[t * g.BR + r] = ytab[(int64_t)t * g.Hr + bd.ry_lo + r];
  }
  // the band's source rows are one contiguous byte range of the NHWC image
  const int64_t row_bytes = (int64_t)g.W * g.C;
  const uint8_t* gsrc = src + (b * g.H + bd.r0) * row_bytes;
  const int nbytes = bd.nrows * (int)row_bytes;
  if ((reinterpret_cast<uintptr_t>(gsrc) & 15) == 0 && (nbytes & 15) == 0) {
    for (int i = tid; i < nbytes / 16; i += nt)
      reinterpret_cast<uint4*>(sl)[i] = reinterpret_cast<const uint4*>(gsrc)[i];
  } else {
    for (int i = tid; i < nbytes; i += nt) sl[i] = gsrc[i];
  }
  __syncthreads();

  // horizontal pass: mid[c][r][rx] = clamp((2^21 + sum_t src[r][start + t][c] * k[t][rx]) >> 22)
  const int hw = bd.nrows * g.Wr;
  for (int i = tid; i < g.C * hw; i += nt) {
    const int c = i / hw, rem = i - c * hw, r = rem / g.Wr, rx = rem - r * g.Wr;
    const int st = min(max(xs[rx], 0), g.W);
    const int cnt = min(xs[g.Wr + rx], g.W - st);
    const uint8_t* s = sl + ((int64_t)r * g.W + st) * g.C + c;
    const int32_t* k = xs + 2 * g.Wr + rx;
    int acc = 1 << 21;
    for (int t = 0; t < cnt; ++t) acc += (int)s[t * g.C] * k[t * g.Wr];
    mid[i] = (uint8_t)min(max(acc >> 22, 0), 255);
  }
  __syncthreads();

  bd.lut = lut;
  bd.xs = xs;
  bd.ys = ys;
  bd.mid = mid;
  return bd;
}

// Vertical pass + crop + flip + normalize: the 4 values of output row y, columns x0..x0+3, channel c.
__device__ __forceinline__ f32x4 resize_quad(const Band& bd, const ResizeGeom& g, int c, int y, int x0) {
  const float* lut = bd.lut + c * 256;
  f32x4 o;
  const int ry = y + bd.dy;
  if (ry < bd.ry_lo || ry >= bd.ry_hi) {
    o[0] = o[1] = o[2] = o[3] = lut[g.fill];
    return o;
  }
  const int j = ry - bd.ry_lo;
  const int base = min(max(bd.ys[j] - bd.r0, 0), bd.nrows);
  const int cnt = min(bd.ys[g.BR + j], bd.nrows - base);
  const int32_t* k = bd.ys + 2 * g.BR + j;
  const uint8_t* m = bd.mid + ((int64_t)c * bd.nrows + base) * g.Wr;
  int rx[4], rc[4], acc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int x = x0 + e;
    rx[e] = (bd.fl ? g.S - 1 - x : x) + bd.dx;
    rc[e] = min(max(rx[e], 0), g.Wr - 1);      // columns outside the resized image read a valid byte, then take fill
    acc[e] = 1 << 21;
  }
  for (int t = 0; t < cnt; ++t, m += g.Wr) {   // one weight per tap for the 4 columns
    const int w = k[t * g.BR];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += (int)m[rc[e]] * w;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = lut[(rx[e] >= 0 && rx[e] < g.Wr) ? min(max(acc[e] >> 22, 0), 255) : g.fill];
  return o;
}

// grid (bands, B): fp32 NCHW [B, C, S, S]
__global__ __launch_bounds__(256) void resize_ingest_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                           const int32_t* __restrict__ ytab, const int32_t* __restrict__ xtab,
                                                           const int32_t* __restrict__ oy, const int32_t* __restrict__ ox,
                                                           const uint8_t* __restrict__ flip, const float* __restrict__ mean,
                                                           const float* __restrict__ stdv, ResizeGeom g) {
  extern __shared__ __align__(16) uint8_t lds[];
  const int64_t b = blockIdx.y;
  const int y0 = blockIdx.x * g.BR, y1 = min(g.S, y0 + g.BR);
  const Band bd = resize_stage(lds, g, src, ytab, xtab, oy, ox, flip, mean, stdv, b, y0, y1);
  const int xq = g.S / 4, rows = y1 - y0;
  for (int i = threadIdx.x; i < g.C * rows * xq; i += blockDim.x) {
    const int x4 = i % xq, t = i / xq, yy = t % rows, c = t / rows;
    const int y = y0 + yy;
    *reinterpret_cast<f32x4*>(dst + ((b * g.C + c) * (int64_t)g.S + y) * g.S + x4 * 4) = resize_quad(bd, g, c, y, x4 * 4);
  }
}

// grid (bands, B): patch rows [B*(cls_rows + (S/p)^2), out_ld], k = c p^2 + i p + j; a band is BR/p whole patch rows
template <typename TD>
__global__ __launch_bounds__(256) void resize_ingest_patchify_kernel(const uint8_t* __restrict__ src, TD* __restrict__ out,
                                                                    int64_t out_ld, const int32_t* __restrict__ ytab,
                                                                    const int32_t* __restrict__ xtab,
                                                                    const int32_t* __restrict__ oy, const int32_t* __restrict__ ox,
                                                                    const uint8_t* __restrict__ flip, const float* __restrict__ mean,
                                                                    const float* __restrict__ stdv, ResizeGeom g, int p,
                                                                    int cls_rows) {
  extern __shared__ __align__(16) uint8_t lds[];
  const int64_t b = blockIdx.y;
  const int y0 = blockIdx.x * g.BR, y1 = min(g.S, y0 + g.BR);
  const Band bd = resize_stage(lds, g, src, ytab, xtab, oy, ox, flip, mean, stdv, b, y0, y1);
  const int gp = g.S / p, ntok = cls_rows + gp * gp, Kp = g.C * p * p, kq = (int)(out_ld / 4);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < cls_rows * kq; i += blockDim.x)
      store4<TD>(out + (b * ntok + i / kq) * out_ld + (i % kq) * 4, zero);
  const int ntk = (y1 - y0) / p * gp;      // tokens of this band
  const int tok0 = cls_rows + y0 / p * gp;
  for (int i = threadIdx.x; i < ntk * kq; i += blockDim.x) {
    const int k4 = i % kq, tk = i / kq;
    const int64_t row = b * ntok + tok0 + tk;
    f32x4 v = zero;
    if (k4 * 4 < Kp) {
      const int pt = tok0 - cls_rows + tk, py = pt / gp, px = pt % gp;
      const int k = k4 * 4, c = k / (p * p), rem = k % (p * p), ii = rem / p, jj = rem % p;
      v = resize_quad(bd, g, c, py * p + ii, px * p + jj);
    }
    store4<TD>(out + row * out_ld + k4 * 4, v);
  }
}

// Fill g (band height, LDS bound) for a launch; returns 0 or a VITMI_E_* code through vitmi_fail.
int resize_geom(ResizeGeom& g, int64_t H, int64_t W, int64_t C, int64_t Hr, int64_t Wr, int64_t ytaps, int64_t xtaps,
                int64_t S, int64_t pad, int64_t fill, int band_unit, size_t* lds_bytes) {
  VITMI_REQUIRE(Hr > 0 && Wr > 0 && ytaps >= 1 && ytaps <= kTapLimit && xtaps >= 1 && xtaps <= kTapLimit, VITMI_E_SHAPE,
                "resize_ingest: tables need 1..%d taps (got %lld, %lld)", kTapLimit, (long long)ytaps, (long long)xtaps);
  VITMI_REQUIRE(C <= 4 && H <= 4096 && W <= 4096 && Hr <= 4096 && Wr <= 4096, VITMI_E_SHAPE,
                "resize_ingest: C <= 4 and sizes <= 4096");
  VITMI_REQUIRE(pad >= 0 && fill >= 0 && fill <= 255 && S <= Hr + 2 * pad && S <= Wr + 2 * pad, VITMI_E_SHAPE,
                "resize_ingest: crop %lld does not fit the padded resized image (%lldx%lld+2*%lld)", (long long)S,
                (long long)Hr, (long long)Wr, (long long)pad);
  g.H = (int)H; g.W = (int)W; g.C = (int)C; g.Hr = (int)Hr; g.Wr = (int)Wr; g.S = (int)S;
  g.pad = (int)pad; g.fill = (int)fill; g.ytaps = (int)ytaps; g.xtaps = (int)xtaps;
  // a band of BR resized rows spans fewer than (BR-1)*H/Hr + ytaps source rows (PIL's windows: centre +- support,
  // support <= (ytaps-1)/2); one row of slack.  Halve the band while the workgroup's LDS does not fit.
  for (int units = band_unit >= 32 ? 1 : 32 / band_unit;; units /= 2) {
    g.BR = units * band_unit;
    g.rows_cap = (int)std::min<int64_t>(H, ((int64_t)(g.BR - 1) * H + Hr - 1) / Hr + ytaps + 1);
    const int total = lds_layout(g).total;
    if (total <= kMaxLds) {
      *lds_bytes = (size_t)total;
      return 0;
    }
    if (units == 1)
      return vitmi_fail(VITMI_E_SHAPE, "resize_ingest: %lldx%lld -> %lldx%lld needs %d B of LDS per workgroup (limit %d)",
                        (long long)H, (long long)W, (long long)Hr, (long long)Wr, total, kMaxLds);
  }
}

}  // namespace

// Host-only: the band height and LDS bytes resize_geom picks for a launch of this geometry, or its refusal.
extern "C" int vitmi_resize_ingest_plan(int64_t H, int64_t W, int64_t C, int64_t Hr, int64_t Wr, int64_t ytaps, int64_t xtaps,
                                        int64_t S, int64_t pad, int64_t fill, int64_t band_unit, int* band_rows,
                                        int64_t* lds_bytes) {
  VITMI_REQUIRE(band_rows && lds_bytes && H > 0 && W > 0 && C > 0 && S > 0 && band_unit > 0 && band_unit <= 64,
                VITMI_E_BADARG, "resize_ingest_plan: bad argument");
  ResizeGeom g;
  size_t lds = 0;
  if (int rc = resize_geom(g, H, W, C, Hr, Wr, ytaps, xtaps, S, pad, fill, (int)band_unit, &lds)) return rc;
  *band_rows = g.BR;
  *lds_bytes = (int64_t)lds;
  return 0;
}

extern "C" int vitmi_resize_ingest(const void* src_u8_nhwc, float* dst_nchw, const int32_t* ytab, int64_t ytaps, int64_t Hr,
                                   const int32_t* xtab, int64_t xtaps, int64_t Wr, const int32_t* off_y, const int32_t* off_x,
                                   const uint8_t* flip, const float* mean, const float* stdv, int64_t B, int64_t H,
                                   int64_t W, int64_t C, int64_t S, int64_t pad, int64_t fill, void* stream_) {
  VITMI_REQUIRE(src_u8_nhwc && dst_nchw && ytab && xtab && B > 0 && H > 0 && W > 0 && C > 0 && S > 0, VITMI_E_BADARG,
                "resize_ingest: bad argument");
  VITMI_REQUIRE(S % 4 == 0 && is_aligned(dst_nchw, 16), VITMI_E_ALIGN,
                "resize_ingest: output size must be a multiple of 4 and dst 16-B aligned");
  VITMI_REQUIRE(B <= 65535, VITMI_E_SHAPE, "resize_ingest: B <= 65535");
  ResizeGeom g;
  size_t lds = 0;
  if (int rc = resize_geom(g, H, W, C, Hr, Wr, ytaps, xtaps, S, pad, fill, 1, &lds)) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const dim3 grid((unsigned)((S + g.BR - 1) / g.BR), (unsigned)B);
  hipLaunchKernelGGL(resize_ingest_kernel, grid, dim3(256), lds, stream, (const uint8_t*)src_u8_nhwc, dst_nchw, ytab, xtab,
                     off_y, off_x, flip, mean, stdv, g);
  return vitmi_check_launch("resize_ingest_kernel");
}

extern "C" int vitmi_resize_ingest_patchify(const void* src_u8_nhwc, void* out, int out_dtype, int64_t out_ld,
                                            const int32_t* ytab, int64_t ytaps, int64_t Hr, const int32_t* xtab,
                                            int64_t xtaps, int64_t Wr, const int32_t* off_y, const int32_t* off_x,
                                            const uint8_t* flip, const float* mean, const float* stdv, int64_t B,
                                            int64_t H, int64_t W, int64_t C, int64_t S, int64_t pad, int64_t fill,
                                            int64_t p, int cls_rows, void* stream_) {
  VITMI_REQUIRE(src_u8_nhwc && out && ytab && xtab && B > 0 && H > 0 && W > 0 && C > 0 && S > 0 && p > 0 && cls_rows >= 0,
                VITMI_E_BADARG, "resize_ingest_patchify: bad argument");
  VITMI_REQUIRE(S % p == 0 && p % 4 == 0 && p <= 64, VITMI_E_SHAPE,
                "resize_ingest_patchify: S %% p and p %% 4 must be 0, p <= 64 (S=%lld p=%lld)", (long long)S, (long long)p);
  if (out_ld == 0) out_ld = C * p * p;
  VITMI_REQUIRE(out_ld >= C * p * p && out_ld % 4 == 0 && out_ld / 4 < (1 << 24) && is_aligned(out, 16), VITMI_E_ALIGN,
                "resize_ingest_patchify: out_ld / alignment");
  VITMI_REQUIRE(B <= 65535, VITMI_E_SHAPE, "resize_ingest_patchify: B <= 65535");
  ResizeGeom g;
  size_t lds = 0;
  if (int rc = resize_geom(g, H, W, C, Hr, Wr, ytaps, xtaps, S, pad, fill, (int)p, &lds)) return rc;
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  const dim3 grid((unsigned)((S + g.BR - 1) / g.BR), (unsigned)B);
#define GO(TD)                                                                                                          \
  hipLaunchKernelGGL((resize_ingest_patchify_kernel<TD>), grid, dim3(256), lds, stream, (const uint8_t*)src_u8_nhwc,      \
                     (TD*)out, out_ld, ytab, xtab, off_y, off_x, flip, mean, stdv, g, (int)p, cls_rows)
  if (out_dtype == VITMI_BF16) GO(bf16);
  else if (out_dtype == VITMI_F32) GO(float);
  else return vitmi_fail(VITMI_E_DTYPE, "resize_ingest_patchify: bad out dtype");
#undef GO
  return vitmi_check_launch("resize_ingest_patchify_kernel");
}
