"""Element-wise error bounds and guarded buffers for the conv / GEMM kernel tests.

ref_and_scale computes an operation in float64 from the operands as the kernel sees them (already rounded to their
storage type) together with its condition scale S = the same operation on |operands|, i.e. S = sum |a * b| per output
element.  check then asserts, element by element,

    |got - ref| <= (1 + u_out) * |scale| * c_acc(K) * S + u_out * |ref| (+ u_out * |pre|) + tiny

where c_acc bounds the f32 accumulation (an exact k-ordered f32 fma chain: 0.75-1.5e-7 * S for K <= 1024 and
3.5e-7 * S at K = 4096, taken as 4e-7 * max(1, K / 1024); bf16 products are exact in f32, so the same term applies),
and u_out is the rounding of the stored value: 2^-8 for bf16 (half an ulp, relative: 8 significant bits), whose
(1 + u_out) factor carries the accumulation error through that rounding; 2^-23 for f32 (two f32 roundings: the bias
add and the scale).  The f32 roundings before a bf16 store (<= 2^-23 |ref|) fit inside |scale| * c_acc * S, because
S >= |acc + bias| = |ref / scale| before ReLU.  `pre` is the value before a second
rounding in storage precision (the residual addend is added to the already-rounded result).  ReLU, the gate and an
explicit keep-mask are 1-Lipschitz or exact, so the same bound covers them.

guarded() hands out outputs inside a buffer of NaN sentinels (a guard band of at least one 128-row tile before and
after the interior, and the columns ncols..ld of every interior row); assert_guards() then asserts that no byte outside
the interior changed and that every interior element was written.  The same buffers, filled with data, serve as
poisoned inputs: a read the ABI does not allow reaches an output as NaN."""
import torch
import torch.nn.functional as F

U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -23}
TINY = 1e-30
# NaN bit patterns that no kernel produces by arithmetic (the default quiet NaN of both types has a zero payload)
SENTINEL = {torch.bfloat16: (torch.int16, 0xFFC1 - 0x10000), torch.float32: (torch.int32, 0x7FC0DEAD)}
GUARD_ROWS = 128


def c_acc(K, dtype=torch.float32):
    """Accumulation error per unit of S for a K-long f32 accumulation (f32 products: an exact fma chain; bf16 products
    are exact in f32 and accumulate the same way)."""
    return 4e-7 * max(1.0, K / 1024.0)


# ---- float64 references -------------------------------------------------------------------------------------------

def _conv2d(x, w, stride=1, padding=1):
    return F.conv2d(x, w, None, stride=stride, padding=padding)


def _conv_transpose2d(x, w, stride=2, padding=1, output_padding=1):
    return F.conv_transpose2d(x, w, None, stride=stride, padding=padding, output_padding=output_padding)


def _linear(a, w):
    return a @ w.t()


def _wgrad_conv2d(dy, x, wshape, stride=1, padding=1):
    """dW[co][ci][kh][kw] of conv2d(x, W) for the output gradient dy."""
    return torch.nn.grad.conv2d_weight(x, wshape, dy, stride=stride, padding=padding)


def _wgrad_conv_transpose2d(dy, x, wshape, stride=2, padding=1):
    """dW[ci][co][kh][kw] of conv_transpose2d(x, W) (x: [N][ci][H][W]): the transposed conv is conv2d's input
    gradient, so its weight gradient is conv2d's with the roles of input and output gradient exchanged."""
    return torch.nn.grad.conv2d_weight(dy, wshape, x, stride=stride, padding=padding)


def _wgrad_linear(dy, x):
    return dy.t() @ x


OPS = {"conv2d": _conv2d, "conv_transpose2d": _conv_transpose2d, "linear": _linear,
       "wgrad_conv2d": _wgrad_conv2d, "wgrad_conv_transpose2d": _wgrad_conv_transpose2d, "wgrad_linear": _wgrad_linear}


def ref_and_scale(op, a, b, **kw):
    """(ref, S) of OPS[op](a, b, **kw) in float64 on the CPU: a and b as the kernel sees them (storage-rounded)."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    f = OPS[op]
    return f(a, b, **kw), f(a.abs(), b.abs(), **kw)


def rows(t):
    """[N][C][H][W] -> NHWC rows [N*H*W][C]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


# ---- the element-wise check ---------------------------------------------------------------------------------------

def bound(ref, S, *, out_dtype, K, scale=1.0, pre=None, S_in=None, u_in=0.0):
    u = U_OUT[out_dtype]
    b = (1 + u) * abs(scale) * c_acc(K) * S + u * ref.abs() + TINY
    if pre is not None:
        b = b + u * pre.abs()
    if S_in is not None:
        b = b + (1 + u) * abs(scale) * u_in * S_in
    return b


def check(got, ref, S, *, out_dtype, K, scale=1.0, pre=None, nhw=None, what="", S_in=None, u_in=0.0):
    """Assert |got - ref| <= bound element-wise; got, ref and S are [rows][C] (NHWC rows when nhw = (N, H, W) is given,
    which maps the worst row back to (image, y, x)).  S_in / u_in: the staged-operand term (staged_u_in).  Returns the
    worst |err| / bound."""
    got = got.detach().cpu().double()
    ref, S = ref.double().reshape(got.shape), S.double().reshape(got.shape)
    if pre is not None:
        pre = pre.double().reshape(got.shape)
    if S_in is not None:
        S_in = S_in.double().reshape(got.shape)
    bnd = bound(ref, S, out_dtype=out_dtype, K=K, scale=scale, pre=pre, S_in=S_in, u_in=u_in)
    err = (got - ref).abs()
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / bnd)
    bad = ~(err <= bnd)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if bool(bad.any()):
        flat = int(torch.argmax(ratio.reshape(-1)))
        r, c = divmod(flat, got.shape[-1]) if got.dim() > 1 else (flat, 0)
        where = f"(row {r}, channel {c})"
        if nhw is not None:
            n, rem = divmod(r, nhw[1] * nhw[2])
            where += f" = (image {n}, y {rem // nhw[2]}, x {rem % nhw[2]}, c {c})"
        g, f = got.reshape(-1)[flat].item(), ref.reshape(-1)[flat].item()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst "
                             f"|err|/bound = {worst:.3g} at {where}: got {g!r}, ref {f!r}, bound {bnd.reshape(-1)[flat]:.3g}")
    return worst


def colsum_bound(vals):
    """Bound of an f32 sum of the rows of vals (any order): (n - 1) * 2^-24 * sum |v| (recursive summation)."""
    return max(vals.shape[0] - 1, 1) * 2.0 ** -24 * vals.abs().sum(0) + TINY


U32 = 2.0 ** -24              # unit roundoff of f32


# ---- an operand computed in the kernel: GroupNorm (+ swish) applied while the input is staged -----------------------

def staged_operand(x, scale, shift, swish):
    """float64 a = swish?(x * scale + shift) of an [N][C][H][W] input (scale / shift [N][C]), NOT rounded to the storage
    type: the reference operand of a kernel that computes a in f32 and rounds it before the MFMA.  Also returns
    max |x * scale + shift| (for staged_u_in)."""
    t = x.double() * scale.double()[:, :, None, None] + shift.double()[:, :, None, None]
    a = t * torch.sigmoid(t) if swish else t
    return a, float(t.abs().max()) if t.numel() else 0.0


def staged_u_in(dtype, swish, tmax):
    """Relative error of the staged operand a against staged_operand's float64 value: u_in = 2^-8 (round to nearest
    bf16) + c_eval for bf16, c_eval for f32 (the f32 value is the MFMA operand).  c_eval, in units u = 2^-24:
      t = fmaf(x, scale, shift): one rounding, |dt| <= u |t|; through swish (|t swish'(t) / swish(t)| <= 1 + |t|):
      (1 + |t|) u.  bf16 swish, t * rcp(1 + exp2(-1.44269504 t)): the constant's and the product's rounding put an
      absolute error of 2 u |1.4427 t| into exp2's argument, i.e. a relative 2 |t| u into e = exp2(..); v_exp_f32 and
      v_rcp_f32 are 1 ulp (2 u) each; 1 + e and the final product one rounding each; a relative error of e moves the
      sigmoid by at most as much: (1 + |t|) + 2 |t| + 2 + 1 + 2 + 1 = 7 + 3 |t|.  f32 swish, t / (1 + expf(-t)):
      expf 1 ulp, 1 + e, the division and the product one rounding each: 6 + |t|.  Without swish: 1.
    c_eval = (8 + 3 tmax) u covers both swish forms, tmax = max |t| of the case."""
    c_eval = (8 + 3 * tmax) * U32 if swish else U32
    return (2.0 ** -8 if dtype == torch.bfloat16 else 0.0) + c_eval


# ---- GroupNorm statistics out of an epilogue ---------------------------------------------------------------------

def stats_height(cg):
    """Additions any one stored value goes through on its way into conv_halo_k's (mean, M2) of a tile and group of cg
    channels (csrc/conv_halo.hip): <= 16 rows per thread, two lane merges, eight waves, cg channels, two divisions;
    the recursive-summation bound of a tree is (height) u sum |terms|."""
    return cg + 28


def tile_stats_bounds(n, cg, sum_abs, amax, m2, h=None):
    """Bounds of the kernel's f32 (mean, M2) of one tile and group: n values (pixels x cg), sum |x|, max |x| and the
    float64 M2 of the stored values.  mean: h u sum|x| / n.  M2: every partial mean is off by at most E = h u max|x|;
    the squared deviations of a partial from its OWN mean cancel that to first order, the merge terms
    n_a n_b / n (mean_a - mean_b)^2 do not: at most 2 E sqrt(W M2) per merge level (Cauchy-Schwarz, W <= n) over <= 4
    levels, plus n E^2 per level and for the threads; the sums of the nonnegative terms (2 h + 4) u M2.
    h: the summation height of another kernel's statistics (default: conv_halo_k's stats_height(cg)); the arguments
    may be tensors of one shape."""
    h = stats_height(cg) if h is None else h
    E = h * U32 * amax
    bm = h * U32 * sum_abs / n + TINY
    bM2 = (2 * h + 4) * U32 * m2 + 8 * E * (n * m2) ** 0.5 + 5 * n * E * E + TINY
    return bm, bM2, E


# ---- guarded buffers ----------------------------------------------------------------------------------------------

class Guarded:
    """A [guard + rows + guard][ld] buffer of sentinels; .view is the [rows][ld] interior handed to a kernel, .out its
    [rows][ncols] part (the declared elements)."""

    def __init__(self, rows, ld, ncols, dtype, guard_rows=GUARD_ROWS, device="cuda", row_align=16):
        ib, pat = SENTINEL[dtype]
        es = torch.empty((), dtype=dtype).element_size()
        assert (ld * es) % row_align == 0, "rows of a guarded buffer keep 16-byte alignment (row_align: a test of a misaligned ld)"
        assert ncols <= ld
        self.rows, self.ld, self.ncols, self.dtype, self.g = rows, ld, ncols, dtype, max(guard_rows, GUARD_ROWS)
        self.buf = torch.full((self.g + rows + self.g, ld), pat, dtype=ib, device=device).view(dtype)
        self.view = self.buf[self.g:self.g + rows]
        self.out = self.view[:, :ncols]
        assert self.view.data_ptr() % 16 == 0

    def fill(self, t):
        """Store t ([rows][ncols], converted to the buffer's type) into the interior; the rest stays sentinel."""
        self.out.copy_(t.reshape(self.rows, self.ncols).to(self.dtype))
        return self


class GuardedFlat(Guarded):
    """n contiguous elements inside `guard` sentinels on each side (packed outputs such as float2 statistics)."""

    def __init__(self, n, dtype, guard=1024, device="cuda"):
        ib, pat = SENTINEL[dtype]
        self.rows, self.ld, self.ncols, self.dtype, self.g = n, 1, 1, dtype, guard
        self.buf = torch.full((guard + n + guard, 1), pat, dtype=ib, device=device).view(dtype)
        self.view = self.buf[guard:guard + n].view(-1)
        self.out = self.view
        assert self.view.data_ptr() % 16 == 0


class GuardedBytes:
    """n bytes starting `offset` bytes past a 256-byte boundary (so .view's address & 3 == offset & 3), inside `guard`
    bytes of `sentinel` on each side.  A legitimate output byte can equal the sentinel, so a byte-exact test runs twice
    with two sentinels: both runs equal to the reference and both pairs of bands intact show that every byte of the
    interior was written and none outside it.  The bands are compared on the device (the buffers of the large cases are
    not copied to the host)."""

    def __init__(self, n, sentinel=0xA5, offset=0, guard=4096, device="cuda"):
        self.n, self.sentinel, self.lo = n, sentinel, guard + offset
        self.buf = torch.full((self.lo + n + guard,), sentinel, dtype=torch.uint8, device=device)
        self.view = self.buf[self.lo:self.lo + n]
        assert self.buf.data_ptr() % 256 == 0 and self.view.data_ptr() % 4 == offset % 4

    def fill(self, t):
        self.view.copy_(t.reshape(-1))
        return self


def assert_byte_bands(g, what=""):
    """Every byte of g.buf outside the interior still holds the sentinel."""
    for name, band, base in (("before", g.buf[:g.lo], -g.lo), ("after", g.buf[g.lo + g.n:], g.n)):
        bad = (band != g.sentinel).nonzero()
        assert bad.shape[0] == 0, (f"{what}: {bad.shape[0]} bytes {name} the output were written; first at byte "
                                   f"{int(bad[0, 0]) + base} relative to the interior")


def assert_bytes_untouched(g, what=""):
    """assert_byte_bands and an interior that is still sentinel: a refused call wrote nothing."""
    assert_byte_bands(g, what)
    bad = (g.view != g.sentinel).nonzero()
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} output bytes were written by a refused call; first at {int(bad[0, 0])}"


def guarded(rows, ld, ncols, dtype, guard_rows=GUARD_ROWS, device="cuda", row_align=16):
    return Guarded(rows, ld, ncols, dtype, guard_rows, device, row_align)


def poisoned(t, ld, dtype, guard_rows=GUARD_ROWS, device="cuda", row_align=16):
    """Input operand t ([rows][ncols]) inside NaN guard rows and NaN padding columns ncols..ld."""
    t = t.reshape(t.shape[0], -1)
    return Guarded(t.shape[0], ld, t.shape[1], dtype, guard_rows, device, row_align).fill(t.to(device))


def assert_guards(g, what=""):
    """Every element outside g's interior still holds the sentinel; no interior element does (all were written)."""
    ib, pat = SENTINEL[g.dtype]
    bits = g.buf.view(ib).cpu()
    sent = bits == pat
    inner = torch.zeros_like(sent)
    inner[g.g:g.g + g.rows, :g.ncols] = True
    stray = (~sent & ~inner).nonzero()
    assert stray.shape[0] == 0, (f"{what}: {stray.shape[0]} elements outside the output were written; first at buffer "
                                 f"(row {int(stray[0, 0]) - g.g}, col {int(stray[0, 1])}) relative to the interior")
    unwritten = (sent & inner).nonzero()
    assert unwritten.shape[0] == 0, (f"{what}: {unwritten.shape[0]} output elements were never written; first at "
                                     f"(row {int(unwritten[0, 0]) - g.g}, col {int(unwritten[0, 1])})")


def assert_guards_where(g, written, what=""):
    """assert_guards for an output that declares only part of its interior (a strided scatter, an offset workspace):
    `written` marks the declared elements of g.view ([rows][ld], or [n] of a GuardedFlat); everything else, inside the
    interior and around it, still holds the sentinel, and every declared element was written."""
    ib, pat = SENTINEL[g.dtype]
    sent = g.buf.view(ib).cpu() == pat
    inner = torch.zeros_like(sent)
    inner[g.g:g.g + g.rows] = written.reshape(g.rows, -1).cpu()
    stray = (~sent & ~inner).nonzero()
    assert stray.shape[0] == 0, (f"{what}: {stray.shape[0]} undeclared elements were written; first at buffer "
                                 f"(row {int(stray[0, 0]) - g.g}, col {int(stray[0, 1])}) relative to the interior")
    unwritten = (sent & inner).nonzero()
    assert unwritten.shape[0] == 0, (f"{what}: {unwritten.shape[0]} declared elements were never written; first at "
                                     f"(row {int(unwritten[0, 0]) - g.g}, col {int(unwritten[0, 1])})")
