"""References, input builders and case lists for the loss, reduction and layout kernels (csrc/elementwise.hip, the GELU
pair of csrc/split3.hip, colsum_mul of csrc/cait_ops.hip, the relative-position, PatchMerging and token-mean kernels of
csrc/swin_ops.hip).  Everything here is float64 or integer torch on the CPU; tests/test_elementwise_ref_cpu.py checks
the references against independent formulations and the conditions the inputs must satisfy, and
tests/test_elementwise_f64_gpu.py runs the kernels against them.

Exact sections: operands are integers in [-8, 8] (exact in bf16), so every partial and final sum is an integer below
2^24 in magnitude: exact in fp32 in any summation order, and the kernel must return the integer reference bit for bit.
"""
import functools
import math

import torch

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
EXACT_LIMIT = 1 << 24          # integers of smaller magnitude are exact in fp32
DT_NAME = {F32: "fp32", BF16: "bf16"}
PAIRS = [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)]
PAIR_IDS = [f"{DT_NAME[a]}-{DT_NAME[b]}" for a, b in PAIRS]


def gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


def ints(shape, seed, lo=-8, hi=8):
    """Integers in [lo, hi] (int64)."""
    return torch.randint(lo, hi + 1, shape, generator=gen(seed))


def normal(shape, seed, scale=1.0):
    return torch.randn(shape, generator=gen(seed)) * scale


def bits(t):
    """The bit pattern of an fp32 / bf16 tensor as integers."""
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def same_bits(got, want):
    """Bitwise equality, except that a NaN equals any NaN (the payload is not part of any contract here)."""
    assert got.dtype == want.dtype and got.shape == want.shape
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn) and torch.equal(bits(got)[~gn], bits(want)[~wn]))


def sum_metric(got, want, denom):
    """max over output elements of |got - want| / (sum of |terms| of that element): a bad column cannot hide behind the
    tensor's largest value.  Elements whose terms are all zero must be exact."""
    d = (got.to(F64) - want.to(F64)).abs()
    assert bool((d[denom == 0] == 0).all())
    return (d / denom.clamp_min(1e-300)).max().item()


# ------------------------------------------------------------------------------------------------------ colsum ---
FOLD_DIRECT_ROWS = 2048        # vitmi_colsum: an fp32 matrix of at most this many rows is folded directly
ROWS_KERNEL_MAX_N = 512        # the rows-per-workgroup kernel serves N <= 512


def colsum_form(dtype, M, N, ld, misaligned=False):
    """The kernel form vitmi_colsum dispatches to (csrc/elementwise.hip, vitmi_colsum)."""
    if dtype == F32 and M <= FOLD_DIRECT_ROWS:
        return "direct"
    vec = N % 4 == 0 and ld % 4 == 0 and not misaligned
    if vec and N <= ROWS_KERNEL_MAX_N:
        return "rows"
    return "vec4" if vec else "scalar"


def rows_per_step(N):
    """R of colsum_partial_rows_kernel: 256 threads tile R consecutive rows of N / 4 column groups."""
    return 256 // (N // 4)


class ColsumCase:
    """x = a [M, N] view at row stride ld, `col0` columns into its rows, `lead` elements into its buffer."""

    def __init__(self, form, dtype, M, N, ld=None, col0=0, lead=0):
        self.form, self.dtype, self.M, self.N, self.ld, self.col0, self.lead = form, dtype, M, N, ld or N, col0, lead

    @property
    def id(self):
        s = f"{self.form}-{DT_NAME[self.dtype]}-M{self.M}-N{self.N}"
        return s + (f"-ld{self.ld}" if self.ld != self.N else "") + (f"-c{self.col0}" if self.col0 else "") \
            + (f"-lead{self.lead}" if self.lead else "")

    def buffer_numel(self):
        return self.lead + self.M * self.ld

    def view(self, buf):
        return buf[self.lead:self.lead + self.M * self.ld].view(self.M, self.ld)[:, self.col0:self.col0 + self.N]

    def misaligned(self):
        return (self.lead + self.col0) % 4 != 0

    def integers(self):
        """The whole buffer as integers in [-8, 8]; what lies outside the view is part of no sum."""
        return ints((self.buffer_numel(),), 7 * self.M + 13 * self.N + self.ld)

    def normals(self):
        return normal((self.buffer_numel(),), 7 * self.M + 13 * self.N + self.ld + 1)


def colsum_cases():
    c = []
    for M in (1, 63, 64, 65, 2048):                                    # direct fold: 64 row groups of fold_rows
        for N in (1, 15, 16, 17, 768):                                 # 16 columns per workgroup
            c.append(ColsumCase("direct", F32, M, N))
    c.append(ColsumCase("direct", F32, 65, 17, ld=24))
    for N in (4, 8, 96, 260, 512):                                     # rows kernel
        R = rows_per_step(N)
        for M in sorted({1, R - 1, R, R + 1, 5000} - {0}):
            c.append(ColsumCase("rows", BF16, M, N))
        for M in (2049, 5000):
            c.append(ColsumCase("rows", F32, M, N))
    for dt in (F32, BF16):
        c.append(ColsumCase("rows", dt, 50176, 96))
        c.append(ColsumCase("rows", dt, 2500, 96, ld=288, col0=96))   # a column slice of a wider matrix
    for N in (516, 768, 2304):                                         # 4-wide partial kernel
        for M in (2049, 4100):
            c += [ColsumCase("vec4", F32, M, N), ColsumCase("vec4", BF16, M, N)]
        c += [ColsumCase("vec4", BF16, 3, N), ColsumCase("vec4", BF16, 777, N)]
    for N in (7, 65, 1001):                                            # scalar partial kernel
        c.append(ColsumCase("scalar", BF16, 33, N))
        c += [ColsumCase("scalar", F32, 2500, N), ColsumCase("scalar", BF16, 2500, N)]
    for dt in (F32, BF16):
        c.append(ColsumCase("scalar", dt, 2500, 768, ld=770))
        c.append(ColsumCase("scalar", dt, 2500, 768, lead=1))          # a view one element into its buffer
    return c


def colsum_accuracy_cases():
    """One case per dispatch form at the largest M of that form."""
    return [ColsumCase("direct", F32, 2048, 768),
            ColsumCase("rows", F32, 50176, 96), ColsumCase("rows", BF16, 50176, 96),
            ColsumCase("vec4", F32, 4100, 2304), ColsumCase("vec4", BF16, 4100, 2304),
            ColsumCase("scalar", F32, 2500, 1001), ColsumCase("scalar", BF16, 2500, 1001)]


FOLD_QUEUE_CASE = (300, 768)       # M, N of the queued fp32 fold


# --------------------------------------------------------------------------------------------------- colsum_mul ---
COLSUM_MUL_SHAPES = [(M, N, N, N) for N in (4, 252, 256, 260, 768) for M in (1, 3, 4, 5, 2049, 4100)] \
    + [(2049, 260, 264, 272)]                                          # M, N, ldx, ldy
COLSUM_MUL_ACCURACY = (4100, 768, 768, 768)


def colsum_mul_integers(M, N, ldx, ldy):
    return ints((M, ldx), 3 * M + N), ints((M, ldy), 3 * M + N + 1)


def colsum_mul_normals(M, N, ldx, ldy):
    return normal((M, ldx), 3 * M + N + 2), normal((M, ldy), 3 * M + N + 3)


# --------------------------------------------------------------------------------------------------- token mean ---
TOKEN_MEAN_FWD = [(3, L, 100) for L in (1, 49, 144)]                   # B, L, C: B * C = 300 = 256 + 44
TOKEN_MEAN_BWD = (16, 49, 768)                                         # 2352 workgroups' worth, capped at 2048
TOKEN_MEAN_ACCURACY = (3, 144, 100)


def token_mean_exact(xi):
    """float32(sum) / float32(L) for integer x [B, L, C]: the sum is exact, the division is one IEEE rounding."""
    return xi.sum(1).to(F32) / torch.tensor(float(xi.shape[1]), dtype=F32)


def token_mean_bwd_ref(dout, L, dtype, B):
    """from_f32(dout / L) broadcast over the L tokens."""
    return (dout / torch.tensor(float(L), dtype=F32)).to(dtype).unsqueeze(1).expand(B, L, dout.shape[1]).contiguous()


# ------------------------------------------------------------------------------------------------------- relpos ---
RELPOS_CASES = [(ws, H) for ws in (2, 7, 12) for H in (1, 3, 24)] + [(7, 300)]      # H = 300: head loop, second trip
RELPOS_ACCURACY = (12, 24)
RELPOS_LIST = 256               # relpos_scatter_kernel keeps at most this many positions per table row


def relpos_index(ws):
    from oracle.swin_ref import relative_position_index
    return relative_position_index(ws)


def relpos_gather_ref(table, idx):
    """bias[h][i][j] = table[index[i][j]][h]"""
    N = idx.shape[0]
    return table[idx.reshape(-1)].view(N, N, -1).permute(2, 0, 1).contiguous()


def relpos_scatter_ref(dbias, idx, T):
    """dtable[t][h] = sum over (i, j) with index[i][j] == t of dbias[h][i][j], in dbias' own (integer or float64) type."""
    H, N = dbias.shape[0], dbias.shape[1]
    return torch.zeros((T, H), dtype=dbias.dtype).index_add_(0, idx.reshape(-1), dbias.permute(1, 2, 0).reshape(N * N, H))


# --------------------------------------------------------------------------------------------------------- cast ---
CAST_N = 4194307                # 4 * 2^20 + 3: 4097 workgroups' worth of 4-element groups, capped at 2048, and a 3-tail


def _bf16_tie_neighbourhood():
    """fp32 values at and on either side of a bf16 rounding tie: 1 + 2^-8 lies halfway between 1 and 1 + 2^-7 (ties to
    the even 1), 1 + 3 * 2^-8 halfway between 1 + 2^-7 and 1 + 2^-6 (ties to the even 1 + 2^-6); and their negatives."""
    out = []
    for tie in (1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8):
        for s in (1.0, -1.0):
            out += [s * (tie - 2.0 ** -23), s * tie, s * (tie + 2.0 ** -23)]
    return out


def cast_specials(dtype):
    fmax = torch.finfo(dtype).max
    v = [0.0, -0.0, math.inf, -math.inf, math.nan, fmax, -fmax]
    if dtype == F32:
        v += _bf16_tie_neighbourhood()
    return torch.tensor(v, dtype=F64).to(dtype)


@functools.lru_cache(maxsize=None)
def cast_input(dtype):
    """Normal draws with the special values planted in the first trip, the second trip and the scalar tail."""
    x = normal((CAST_N,), 41).to(dtype)
    sp = cast_specials(dtype)
    n = sp.numel()
    second_trip = 4 * 2048 * 256                      # the first element of the grid-stride loop's second trip
    for at in (0, 1001, second_trip + 5, CAST_N - 3 - n):
        x[at:at + n] = sp
    x[CAST_N - 3:] = torch.tensor([math.nan, -0.0, torch.finfo(dtype).max], dtype=F64).to(dtype)
    return x


def bf16_rne_bits(x32):
    """Round-to-nearest-even fp32 -> bf16 in integer arithmetic (NaN stays NaN): the independent formulation of
    torch's .to(bfloat16) that the CPU test compares it with.  Returns the 16 bits as int32."""
    b = x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    nan = torch.isnan(x32)
    r = torch.where(nan, (b >> 16) | 0x40, r)
    return (r & 0xFFFF).to(torch.int32)


# ----------------------------------------------------------------------------------------------------- patchify ---
PATCHIFY_CASE = (16, 3, 224, 16, 1)       # B, C, H = W, p, cls rows: 2364 workgroups' worth, capped at 2048
PATCHIFY_PAD_LD = 800


def patchify_ref(x, p, cls_rows, ld=None):
    """[B * (cls + gh * gw), ld]: row (b, t) = patch t - cls of image b flattened as (c, i, j); the cls row and the
    columns past C * p * p are zeros."""
    B, C, H, W = x.shape
    gh, gw = H // p, W // p
    rows = x.reshape(B, C, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, C * p * p)
    out = torch.zeros((B, cls_rows + gh * gw, ld or C * p * p), dtype=x.dtype)
    out[:, cls_rows:, :C * p * p] = rows
    return out.reshape(B * (cls_rows + gh * gw), -1)


# -------------------------------------------------------------------------------------------------- patch merge ---
PATCH_MERGE_CASES = [(8, 56, 56, 96), (2, 6, 10, 4)]      # B, H, W, C: 2352 workgroups' worth (cap 2048); a small odd one


def patch_merge_ref(x, B, Hh, Ww, C):
    """out[b, (i, j), k * C + c] = x[b, (2 i + dy_k, 2 j + dx_k), c], k <-> (dy, dx) = (0,0), (1,0), (0,1), (1,1)."""
    out = torch.empty((B, Hh // 2, Ww // 2, 4, C), dtype=x.dtype)
    xv = x.view(B, Hh, Ww, C)
    for k, (dy, dx) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        for i in range(Hh // 2):
            out[:, i, :, k] = xv[:, 2 * i + dy, dx::2]
    return out.view(B, Hh * Ww // 4, 4 * C)


# --------------------------------------------------------------------------------------------------- scale_cast ---
SCALE_CAST_SHAPE = (2100, 1024, 100)      # M, N, rows per group: 2100 workgroups' worth, capped at 2048
SCALE_CAST_LDX, SCALE_CAST_LDO = 1032, 1036
SCALE_FORMS = {"col": (True, False), "row": (False, True), "both": (True, True), "neither": (False, False)}


def scale_cast_inputs(xdt):
    M, N, rpg = SCALE_CAST_SHAPE
    x = normal((M, SCALE_CAST_LDX), 51).to(xdt)
    col = normal((N,), 52)
    row = normal(((M + rpg - 1) // rpg,), 53)
    row[3] = 0.0                                   # a dropped sample
    return x, col, row


def scale_cast_ref(x, col, row, rpg, odt):
    """The kernel's two IEEE fp32 multiplies in its order, (x * scale) * rowscale, then the cast."""
    v = x.to(F32)
    if col is not None:
        v = v * col
    if row is not None:
        v = v * row.repeat_interleave(rpg)[:v.shape[0], None]
    return v.to(odt)


# --------------------------------------------------------------------------------------------------------- axpy ---
AXPY_N = CAST_N
AXPY_A = (1.0, -0.5, 3.0e-3)


@functools.lru_cache(maxsize=None)
def axpy_inputs():
    return normal((AXPY_N,), 61), normal((AXPY_N,), 62)


def axpy_ref(x, y, a):
    """float64 y + a x with the fp32 value of a the kernel receives, and the per-element bound 2^-23 (|y| + |a x|):
    two roundings (product, sum) or one (fused) of at most 2^-24 relative each."""
    a32 = torch.tensor(a, dtype=F32).to(F64)
    ax = a32 * x.to(F64)
    return y.to(F64) + ax, 2.0 ** -23 * (y.to(F64).abs() + ax.abs())


# --------------------------------------------------------------------------------------------------------- gelu ---
GELU_BIG = (2112, 2048)                   # 4224 workgroups' worth of 4-element groups, capped at 4096
GELU_SMALL = (5, 12, 16, 20, 24)          # M, N, ldp, ldd, ldo
GELU_POINTS = [0.0, -0.0, 1e-4, -1e-4, 0.5, -0.5, 3.0, -3.0, 6.0, -6.0]


def gelu_inputs(M, N, seed):
    """pre: the named points, a uniform grid over [-12, 12], normal draws, the named points again (the last row lies in
    the second trip of the capped grid); dh uniform in [-1, 1]."""
    n, k = M * N, len(GELU_POINTS)
    body = n - 2 * k
    pts = torch.tensor(GELU_POINTS, dtype=F32)
    pre = torch.cat([pts, torch.linspace(-12.0, 12.0, body // 2, dtype=F64).to(F32), normal((body - body // 2,), seed, 2.0), pts])
    dh = torch.rand((M, N), generator=gen(seed + 1)) * 2 - 1
    return pre.view(M, N), dh


def gelu_ref(pre, dh):
    """float64 erf GELU and dh * GELU'."""
    x, g = pre.to(F64), dh.to(F64)
    cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return x * cdf, g * (cdf + x * pdf)


def gelu_metric(got, want, pre):
    return ((got.to(F64) - want).abs() / pre.to(F64).abs().clamp_min(1.0)).max().item()


def gelu_torch_f32(pre, dh):
    """torch's float32 CPU F.gelu and its autograd: what the bound is measured from."""
    p = pre.clone().requires_grad_(True)
    y = torch.nn.functional.gelu(p)
    y.backward(dh)
    return y.detach(), p.grad


# --------------------------------------------------------------------------------------------------------- xent ---
class XentRef:
    """float64 log_softmax answers in the kernel's layout: loss [1 + B], correct [1 + B], dlogits [B, K]."""

    def __init__(self, logits, labels):
        B, K = logits.shape
        lp = torch.log_softmax(logits.to(F64), -1)
        ok = (labels >= 0) & (labels < K)
        safe = torch.where(ok, labels, torch.zeros_like(labels))
        rows = torch.where(ok, -lp.gather(1, safe[:, None])[:, 0], torch.full((B,), math.nan, dtype=F64))
        onehot = torch.zeros((B, K), dtype=F64)
        onehot[ok, labels[ok]] = 1.0
        self.loss = torch.cat([rows.mean()[None], rows])
        self.dlogits = (lp.exp() - onehot) / B
        hit = (first_argmax(logits) == labels) & ok
        self.correct = torch.cat([hit.sum()[None], hit.to(torch.int64)]).to(torch.int32)


def first_argmax(logits):
    """The lowest index at which each row attains its maximum."""
    K = logits.shape[1]
    at = logits == logits.max(-1, keepdim=True).values
    return torch.where(at, torch.arange(K)[None, :], torch.full((1, 1), K)).min(-1).values


def xent_errors(loss, dlogits, want):
    """losses relative to max(1, |loss_b|) (NaN rows must be NaN on both sides), dlogits relative to 1 / B."""
    B = dlogits.shape[0]
    wn = torch.isnan(want.loss)
    assert torch.equal(torch.isnan(loss), wn), "NaN losses differ from the reference's"
    l, w = loss.to(F64)[~wn], want.loss[~wn]
    e_loss = ((l - w).abs() / w.abs().clamp_min(1.0)).max().item() if l.numel() else 0.0
    return {"loss": e_loss, "dlogits": ((dlogits.to(F64) - want.dlogits).abs().max() * B).item()}


def xent_torch_f32(logits, labels):
    """torch's float32 CPU cross entropy and its autograd, in the kernel's layout (valid labels only)."""
    lg = logits.clone().requires_grad_(True)
    rows = torch.nn.functional.cross_entropy(lg, labels, reduction="none")
    rows.mean().backward()
    return torch.cat([rows.detach().mean()[None], rows.detach()]), lg.grad


def quantized_logits(B, K, seed, scale=3.0):
    """Normal logits rounded to multiples of 2^-8 and clamped to [-12, 12]: adding +-3e4 (a multiple of 2^-8 whose fp32
    spacing is 2^-9) and multiplying by 1e4 (39.0625 per step) are then exact in fp32."""
    return (normal((B, K), seed, scale).clamp(-12, 12) * 256).round() / 256


def labels_for(B, K, seed):
    return torch.randint(0, K, (B,), generator=gen(seed))


def xent_sweep_cases():
    """(B, K) of the batch and class sweeps: 4 samples per workgroup, 256 per trip of the one-block reduction, 64
    classes per trip of a lane."""
    return [(B, 10) for B in (1, 3, 4, 5, 255, 256, 257, 1030)] + [(7, K) for K in (1, 2, 63, 64, 65, 1000, 1001)]


def xent_sweep_inputs(B, K):
    return normal((B, K), 100 * B + K, 3.0), labels_for(B, K, 100 * B + K + 1)


XENT_TIE_K = 130
XENT_TIE_VALUE = 5.0


def xent_tie_inputs():
    """One row per (tie pattern, label choice).  The tied maximum 5.0 sits at k and k + 1 (different lanes), k and
    k + 64 (the same lane, successive trips), and at three indices mixing both; the label is the first tied index, a
    later one, or none of them.  Everything else is at most 2."""
    K = XENT_TIE_K
    patterns = [(0, 1), (0, 64), (0, 1, 64), (0, 64, 65), (0, 1, 2)]
    rows, labels, ties = [], [], []
    for pi, offs in enumerate(patterns):
        for choice in ("first", "later", "none"):
            k = 3 + 7 * len(rows) % 60
            idx = [k + o for o in offs]
            row = quantized_logits(1, K, 500 + len(rows), 1.0)[0].clamp(max=2.0)
            row[idx] = XENT_TIE_VALUE
            rows.append(row)
            ties.append(idx)
            labels.append({"first": idx[0], "later": idx[-1], "none": (idx[-1] + 17) % K}[choice])
    return torch.stack(rows), torch.tensor(labels), ties


XENT_SCALE_SHAPE = (16, 10)
XENT_SHIFT = 3.0e4
XENT_LSE_SWITCH = 16.0                   # xent_kernel: rows with |lse| at or beyond it are worked relative to their maximum
XENT_SWITCH_SHIFTS = (10.0, -21.5)       # shifts that put some rows of the scale case on either side of the switch
XENT_UNDERFLOW_GAP = 3.0 / 256           # x 1e4 = 117 > 104: exp(-117) is below the smallest fp32 denormal


def xent_scale_inputs():
    B, K = XENT_SCALE_SHAPE
    return quantized_logits(B, K, 77), labels_for(B, K, 78)


def xent_neginf_inputs():
    """One -inf logit per row, never at the label."""
    B, K = 9, 70
    logits, labels = normal((B, K), 81, 3.0), labels_for(B, K, 82)
    at = (labels + 1 + torch.arange(B) * 7) % K
    at = torch.where(at == labels, (at + 1) % K, at)
    logits[torch.arange(B), at] = -math.inf
    return logits, labels, at


def xent_bad_label_inputs():
    """Labels -1 and K in rows 2 and 5 of an 8-row batch."""
    B, K = 8, 10
    logits, labels = normal((B, K), 91, 3.0), labels_for(B, K, 92)
    labels[2], labels[5] = -1, K
    return logits, labels, [2, 5]


# ------------------------------------------------------- the float32-on-CPU measurements the bounds come from ---
def measure_colsum_f32():
    worst = 0.0
    for c in colsum_accuracy_cases():
        x = c.view(c.normals().to(c.dtype))
        want, denom = x.to(F64).sum(0), x.to(F64).abs().sum(0)
        worst = max(worst, sum_metric(x.to(F32).sum(0), want, denom))
    return worst


def measure_colsum_mul_f32():
    M, N, ldx, ldy = COLSUM_MUL_ACCURACY
    worst = 0.0
    for xdt, ydt in PAIRS:
        x, y = colsum_mul_normals(M, N, ldx, ldy)
        x, y = x.to(xdt), y.to(ydt)
        prod = x.to(F64) * y.to(F64)
        worst = max(worst, sum_metric((x.to(F32) * y.to(F32)).sum(0), prod.sum(0), prod.abs().sum(0)))
    return worst


def token_mean_accuracy_input(dtype):
    B, L, C = TOKEN_MEAN_ACCURACY
    return normal((B, L, C), 71).to(dtype)


def measure_token_mean_f32():
    worst = 0.0
    for dt in (F32, BF16):
        x = token_mean_accuracy_input(dt)
        L = x.shape[1]
        worst = max(worst, sum_metric(x.to(F32).mean(1), x.to(F64).mean(1), x.to(F64).abs().sum(1) / L))
    return worst


def relpos_accuracy_input():
    ws, H = RELPOS_ACCURACY
    return normal((H, ws * ws, ws * ws), 73)


def measure_relpos_scatter_f32():
    ws, H = RELPOS_ACCURACY
    idx, T, db = relpos_index(ws), (2 * ws - 1) ** 2, relpos_accuracy_input()
    return sum_metric(relpos_scatter_ref(db, idx, T), relpos_scatter_ref(db.to(F64), idx, T),
                      relpos_scatter_ref(db.to(F64).abs(), idx, T))


def gelu_cases():
    M, N = GELU_BIG
    return [gelu_inputs(M, N, 31), gelu_inputs(GELU_SMALL[0], GELU_SMALL[1], 33)]


def measure_gelu_f32():
    e = {"fwd": 0.0, "bwd": 0.0}
    for pre, dh in gelu_cases():
        wy, wg = gelu_ref(pre, dh)
        y, g = gelu_torch_f32(pre, dh)
        e["fwd"] = max(e["fwd"], gelu_metric(y, wy, pre))
        e["bwd"] = max(e["bwd"], gelu_metric(g, wg, pre))
    return e


def xent_accuracy_inputs():
    """Every (name, logits, labels) of the accuracy cases with valid labels and finite logits."""
    out = [(f"B{B}K{K}", *xent_sweep_inputs(B, K)) for B, K in xent_sweep_cases()]
    lt, yt, _ = xent_tie_inputs()
    out.append(("ties", lt, yt))
    ls, ys = xent_scale_inputs()
    out += [("base", ls, ys), ("x1e4", ls * 1e4, ys), ("+3e4", ls + XENT_SHIFT, ys), ("-3e4", ls - XENT_SHIFT, ys)]
    out += [(f"{s:+.1f}", ls + s, ys) for s in XENT_SWITCH_SHIFTS]
    return out


def measure_xent_f32():
    e = {"loss": 0.0, "dlogits": 0.0}
    for _, logits, labels in xent_accuracy_inputs():
        loss, dl = xent_torch_f32(logits, labels)
        for k, v in xent_errors(loss, dl, XentRef(logits, labels)).items():
            e[k] = max(e[k], v)
    return e
