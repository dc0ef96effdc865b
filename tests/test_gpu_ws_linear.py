"""GPU: the weight-stationary 256 x 256 linear layer (e3dge_ws_linear, csrc/siren_ws.hip) one launch at a time, and the small kernels
that feed the same path (e3dge_ws_pack, e3dge_ws_rowdot2, e3dge_amax, e3dge_amax_rows), each against float64 on the CPU.

The reference is the header's formula restated in torch:

    y = post( W @ pre(x * xmul * x_scale) + bias + colw * pre(m) + r1 + r2 )

The tolerance is PER ROW.  With  bound_p = max_f ( |W| @ |pre(x_p)| + |bias| + |colw m_p| + |r1_p| + |r2_p| )_f  -- the size of what was
summed for row p (r1 is left out for post 3, where it only selects the slope) -- and e32_p the deviation from float64 of the same
formula evaluated in fp32 by torch on the CPU, every row must satisfy

    err_p <= 3 e32_p + 1e-6 bound_p

(the form of test_fuse_sft_mlp_native_against_float64, per row: a cancelling row is not punished, a small row is not excused).
The worst err_p / bound_p of every case goes to the record file next to the fp32 figure.

Leaky relu (post 1) has a kink: entries whose float64 pre-activation is within 1e-5 bound_p of zero are not compared; their share is
capped at 0.1 % (1.5e-4 to 2.5e-4 of the entries of these inputs fall there, in float64 alone) and recorded.  post 3 takes its pattern from r1, an
input, so nothing is excluded there."""
import numpy as np
import pytest
import torch

from conftest import maxerr, record

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib
from e3dge_amd.local_query import _ws_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GROUP = 64                      # rows of one group of ws_linear_kernel
WALK2 = 16384 + 64 + 37         # 258 groups on 256 workgroups: two of them take a second group, the last group is ragged
WALK3 = 32769                   # 513 groups: workgroup 0 takes three (its LDS buffer index returns to 0) with one live row in the tail


def _still_seven(t):
    return maxerr(t, torch.full_like(t, 7.0)) == 0.0


def f32(v):
    """The value the C struct carries (slope, w_fuse and x_scale are floats there)."""
    return float(np.float32(v))


def _weights(seed, span=None):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(256, 256, generator=g) * (1.5 / 16)
    if span is not None:                                    # magnitudes log-uniform over `span`, random signs
        lo, hi = np.log(span[0]), np.log(span[1])
        w = torch.sign(w) * torch.exp(torch.rand(256, 256, generator=g) * (hi - lo) + lo)
    return w


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _place(block, ld=None, off=0, tall=0, junk=3.0, tall_value=None, seed=99):
    """`block` (n, w) as columns [off, off + w) of a (n + tall, ld) device buffer whose other entries are noise of size `junk` (a load
    from the wrong pitch or offset then reads something else); the `tall` extra rows hold `tall_value` where given."""
    n, w = block.shape
    ld = w if ld is None else ld
    full = _randn(seed, n + tall, ld) * junk
    full[:n, off:off + w] = block
    if tall and tall_value is not None:
        full[n:] = tall_value
    return full.to(DEV), ld, off


def _ws(wimg, n_rows, x, y, bias=None, col=None, r1=None, r2=None, xmul=None, x_scale=0.0, pre_relu=False, post=0, slope=0.0, w_fuse=0.0,
        amax_out=None):
    """One e3dge_ws_linear launch.  x, y, r1, r2, xmul: (buffer, ld, off); col: (colw, m buffer, ld_m, off_m)."""
    a = _lib.WsLinear()
    a.wimg, a.bias, a.amax_out = wimg, bias, amax_out
    a.n_rows = n_rows
    a.x, a.ld_x, a.off_x = x
    a.y, a.ld_y, a.off_y = y
    if col is not None:
        a.colw, a.m, a.ld_m, a.off_m = col
    if r1 is not None:
        a.r1, a.ld_r1, a.off_r1 = r1
    if r2 is not None:
        a.r2, a.ld_r2, a.off_r2 = r2
    if xmul is not None:
        a.xmul, a.ld_xmul, a.off_xmul = xmul
    a.x_scale, a.pre_relu, a.post, a.slope, a.w_fuse = x_scale, int(pre_relu), post, slope, w_fuse
    _lib.launch("e3dge_ws_linear", a)


def _formula(dt, W, x, bias=None, colw=None, m=None, r1=None, r2=None, xmul=None, x_scale=0.0, pre_relu=False, post=0, slope=0.0,
             w_fuse=0.0):
    """The header's formula in dtype `dt` on the CPU.  Returns (y, pre-activation of post 0 / 1 or None, bound per row)."""
    c = lambda t: None if t is None else t.to(dt)
    W, x, bias, colw, m, r1, r2, xmul = map(c, (W, x, bias, colw, m, r1, r2, xmul))
    xs = 1.0 if x_scale == 0.0 else f32(x_scale)
    slope, w_fuse = f32(slope), f32(w_fuse)
    if xmul is not None:
        x = x * (xmul * xs)
    elif xs != 1.0:
        x = x * xs
    if pre_relu:
        x = x.clamp_min(0)
    v = x @ W.t()
    bound = x.abs() @ W.abs().t()
    if bias is not None:
        v = v + bias
        bound = bound + bias.abs()
    if colw is not None:
        mm = (m.clamp_min(0) if pre_relu else m)[:, None]
        v = v + colw * mm
        bound = bound + (colw * mm).abs()
    e1 = torch.zeros_like(v) if r1 is None else r1
    e2 = torch.zeros_like(v) if r2 is None else r2
    bound = bound + e2.abs() + (e1.abs() if post != 3 else 0.0)
    pre = None
    if post == 2:
        y = e1 + w_fuse * (e1 * e2 + v)
    elif post == 3:
        y = v * torch.where(r1 > 0, 1.0, slope).to(dt) + e2
    elif post == 4:
        y = v + e1 * (1.0 + w_fuse * e2)
    else:
        y = pre = v + e1 + e2
        if post == 1:
            y = torch.where(pre > 0, pre, pre * slope)
    return y, pre, bound.max(dim=1).values


def _judge(name, got, W, x, **kw):
    """Hold `got` (n, 256) to the per-row bound; records and returns the worst ratios."""
    y64, pre64, bound = _formula(torch.float64, W, x, **kw)
    y32 = _formula(torch.float32, W, x, **kw)[0].double()
    got = got.detach().cpu().double()
    assert got.shape == y64.shape, (tuple(got.shape), tuple(y64.shape))
    d, d32 = (got - y64).abs(), (y32 - y64).abs()
    excluded = 0.0
    if kw.get("post", 0) == 1:                              # the kink: a pre-activation within rounding of zero may sit on the other side
        near = pre64.abs() <= 1e-5 * bound[:, None]
        excluded = float(near.double().mean())
        assert excluded <= 1e-3, (name, excluded)
        d, d32 = d.masked_fill(near, 0.0), d32.masked_fill(near, 0.0)
    d = torch.nan_to_num(d, nan=float("inf"))               # a NaN where float64 has a number is an error, not a pass
    err, e32 = d.max(dim=1).values, d32.max(dim=1).values
    safe = bound.clamp_min(1e-300)
    worst, worst32 = float((err / safe).max()), float((e32 / safe).max())
    record("ws_linear_" + name, rows=got.shape[0], worst_err_over_bound=worst, fp32_cpu_over_bound=worst32, kink_excluded_share=excluded)
    print(f"ws_linear {name}: rows {got.shape[0]} err/bound {worst:.3e} fp32/bound {worst32:.3e} excluded {excluded:.2e}")
    bad = err > 3 * e32 + 1e-6 * bound
    if bool(bad.any()):
        p = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {len(bad)} rows over the bound; first row {p}: err {float(err[p]):.3e}, "
                             f"fp32 {float(e32[p]):.3e}, bound {float(bound[p]):.3e}")
    return worst, worst32


def _ops(n, seed, mag=1.0):
    """The operand blocks of a case on the CPU (every launch picks what it needs)."""
    s = 1000 * seed
    r1 = _randn(s + 3, n, 256) * mag
    return dict(x=_randn(s + 1, n, 256) * mag, xmul=_randn(s + 2, n, 256), r1=r1, r2=_randn(s + 4, n, 256) * mag, m=_randn(s + 5, n) * mag,
                bias=_randn(s + 6, 256) * 0.3 * mag, colw=_randn(s + 7, 256) * 0.3)


def _run_dense(wimg, n, o, use, y_fill=None, **flags):
    """Launch on dense (pitch 256) buffers with the operands named in `use`; returns y (n, 256) and the reference's keyword arguments."""
    dev = lambda t: t.to(DEV).contiguous()
    y = torch.full((n, 256), 7.0 if y_fill is None else y_fill, device=DEV)
    kw, ref = {}, {}
    if "bias" in use:
        kw["bias"] = dev(o["bias"])
        ref["bias"] = o["bias"]
    if "col" in use:
        kw["col"] = (dev(o["colw"]), dev(o["m"]), 1, 0)
        ref["colw"], ref["m"] = o["colw"], o["m"]
    for k in ("r1", "r2", "xmul"):
        if k in use:
            kw[k] = (dev(o[k]), 256, 0)
            ref[k] = o[k]
    _ws(wimg, n, (dev(o["x"]), 256, 0), (y, 256, 0), **kw, **flags)
    return y, dict(ref, **flags)


@pytest.fixture(scope="module")
def layer():
    W = _weights(7)
    return W, _ws_image(W.to(DEV))


# ---------------------------------------------------------------------------------------------------------------------
# 1. every form, one launch each
# ---------------------------------------------------------------------------------------------------------------------
FORMS = {
    "post0_bias": (("bias",), dict()),
    "post0_r1_r2": (("bias", "r1", "r2"), dict()),
    "post1_slope0.2": (("bias",), dict(post=1, slope=0.2)),
    "post1_slope0": (("bias", "r1"), dict(post=1, slope=0.0)),
    "post1_slope1": (("bias",), dict(post=1, slope=1.0)),
    "post2_fuse0.7": (("bias", "r1", "r2"), dict(post=2, w_fuse=0.7)),
    "post3_slope0.2": (("r1", "r2"), dict(post=3, slope=0.2)),
    "post3_slope0": (("bias", "r1"), dict(post=3, slope=0.0)),
    "post4": (("r1", "r2"), dict(post=4, w_fuse=0.7)),
    "pre_relu": (("bias",), dict(pre_relu=True)),
    "col": (("bias", "col"), dict()),
    "pre_relu_col": (("bias", "col", "r1"), dict(pre_relu=True)),
    "xmul_scale0.7": (("xmul", "r1"), dict(x_scale=0.7, post=3, slope=0.2)),
    "xmul_scale_unset": (("xmul", "bias"), dict(x_scale=0.0)),
    "scale0.7_no_xmul": (("bias",), dict(x_scale=0.7)),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_per_row(layer, form):
    """One launch per post / pre / operand combination at 1, 63, 64, 65 and 130 rows (one group ragged and full, a second group).  For
    post 3, r1 carries exact zeros and negative zeros (both take the slope: the reference is r1 > 0); m is negative on half the rows
    under pre_relu."""
    W, wimg = layer
    use, flags = FORMS[form]
    for n in (1, 63, 64, 65, 130):
        o = _ops(n, seed=n + len(form))
        if flags.get("post") == 3:
            flat = o["r1"].view(-1)
            flat[0::7] = 0.0
            flat[3::7] = -0.0
            assert bool((flat == 0).any()) and bool(torch.signbit(flat[flat == 0]).any())
        if "col" in use and flags.get("pre_relu") and n > 1:
            assert bool((o["m"] < 0).any()) and bool((o["m"] > 0).any())
        y, ref = _run_dense(wimg, n, o, use, **flags)
        _judge(form, y, W, o["x"], **ref)


# ---------------------------------------------------------------------------------------------------------------------
# 2. layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off_x", [0, 257])
def test_pitches_offsets_and_the_untouched_surroundings(layer, off_x):
    """x at pitch 513 (offsets 0 and 257: 4-byte aligned rows), r1 at pitch 513 offset 257, m at pitch 513 offset 256, y into columns
    [3, 259) of a 301-wide buffer full of 7.0 with a guard region behind the last row: the block meets the per-row bound and everything
    else still holds 7.0."""
    W, wimg = layer
    n, guard = 130, 70
    o = _ops(n, seed=31 + off_x)
    xb = _place(o["x"], 513, off_x, seed=1)
    r1b = _place(o["r1"], 513, 257, seed=2)
    r2b = _place(o["r2"], 301, 45, seed=3)
    mb = _place(o["m"][:, None], 513, 256, seed=4)
    bias, colw = o["bias"].to(DEV), o["colw"].to(DEV)
    wide = torch.full((n + guard, 301), 7.0, device=DEV)
    _ws(wimg, n, xb, (wide, 301, 3), bias=bias, col=(colw, mb[0], 513, 256), r1=r1b, r2=r2b, pre_relu=True)
    _judge(f"layout_off_x{off_x}", wide[:n, 3:259], W, o["x"], bias=o["bias"], colw=o["colw"], m=o["m"], r1=o["r1"], r2=o["r2"], pre_relu=True)
    assert _still_seven(wide[:n, :3]) and _still_seven(wide[:n, 259:])
    assert _still_seven(wide[n:])                         # nothing behind the last row


@pytest.mark.parametrize("post", [0, 1, 3])
def test_y_may_alias_r2(layer, post):
    """y == r2 (the in-place dx accumulation of the backward chain, pitch 513 offset 257): the same bits as the launch with a separate y."""
    W, wimg = layer
    n = 130
    o = _ops(n, seed=41 + post)
    xb = _place(o["x"], 513, 0, seed=5)
    r1b = _place(o["r1"], 513, 257, seed=6)
    acc0 = _place(o["r2"], 513, 257, seed=7)[0]
    flags = dict(post=post, slope=0.2)
    sep = torch.full((n, 513), 7.0, device=DEV)
    _ws(wimg, n, xb, (sep, 513, 257), r1=r1b, r2=(acc0, 513, 257), **flags)
    acc = acc0.clone()
    _ws(wimg, n, xb, (acc, 513, 257), r1=r1b, r2=(acc, 513, 257), **flags)
    assert torch.equal(acc[:, 257:], sep[:, 257:])
    assert torch.equal(acc[:, :257], acc0[:, :257])                            # the columns in front of the block are left alone
    _judge(f"alias_r2_post{post}", acc[:, 257:], W, o["x"], r1=o["r1"], r2=o["r2"], **flags)


def test_y_may_alias_r1_and_launches_repeat_bit_for_bit(layer):
    """The `de` accumulation (r1 = y, post 0) gives the bits of the launch with a separate y; two launches on the same inputs agree."""
    W, wimg = layer
    n = 130
    o = _ops(n, seed=51)
    x = o["x"].to(DEV)
    de0 = o["r1"].to(DEV)
    sep, sep2 = torch.empty(n, 256, device=DEV), torch.full((n, 256), 7.0, device=DEV)
    _ws(wimg, n, (x, 256, 0), (sep, 256, 0), r1=(de0, 256, 0))
    _ws(wimg, n, (x, 256, 0), (sep2, 256, 0), r1=(de0, 256, 0))
    de = de0.clone()
    _ws(wimg, n, (x, 256, 0), (de, 256, 0), r1=(de, 256, 0))
    assert torch.equal(sep, sep2)
    assert torch.equal(de, sep)
    _judge("alias_r1", de, W, o["x"], r1=o["r1"])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the per-row operand scale
# ---------------------------------------------------------------------------------------------------------------------
def test_rows_from_1e_minus_30_to_1e_plus_25(layer):
    """256 rows of one tensor with magnitudes log-uniform from 1e-30 to 1e+25 (the gradients of the backward chain span many orders of
    magnitude): every row keeps the bound of ITS size.  The residual of a row has the row's magnitude, and there is no bias, so the
    bound of a small row is small."""
    W, wimg = layer
    n = 256
    mag = torch.logspace(-30, 25, n)[torch.randperm(n, generator=torch.Generator().manual_seed(3))][:, None]
    o = _ops(n, seed=61)
    o["x"], o["r1"] = o["x"] * mag, o["r1"] * mag
    y, ref = _run_dense(wimg, n, o, ("r1",))
    _judge("rows_1e-30_to_1e25", y, W, o["x"], **ref)
    y, ref = _run_dense(wimg, n, o, ("r1",), post=3, slope=0.2)
    _judge("rows_1e-30_to_1e25_post3", y, W, o["x"], **ref)


def test_blocks_far_below_their_rows_maximum(layer):
    """Rows in which one 32-column block is 2^-8 / 2^-20 / 2^-30 of the others, and rows in which ALL BUT one block are: a block is
    converted with the scale of its own maximum and rescaled to the row's by an exact power of two; 2^-30 is flushed, which drops less
    than 2^-24 of the row's bound."""
    W, wimg = layer
    n = 96
    o = _ops(n, seed=71)
    x = o["x"].view(n, 8, 32)
    for p in range(n):
        ratio = 2.0 ** -(8, 20, 30)[p % 3]
        blk = (p // 3) % 8
        if p < 48:
            x[p, blk] *= ratio
        else:
            keep = x[p, blk].clone()
            x[p] *= ratio
            x[p, blk] = keep
    y, ref = _run_dense(wimg, n, o, ())
    _judge("block_ratios", y, W, o["x"], **ref)


def test_zero_rows_give_exactly_the_other_terms(layer):
    """An all-zero row of x gives (bias + r1) + r2 to the bit, also when it is the only zero row of its tile or every row but one is
    zero; the one live row of an otherwise zero tensor meets its bound."""
    W, wimg = layer
    n = 130
    o = _ops(n, seed=81)
    rest = ((o["bias"] + o["r1"]) + o["r2"]).to(DEV)
    for name, live in (("one_zero_row", [p for p in range(n) if p != 37]), ("one_live_row", [70])):
        oo = dict(o, x=torch.zeros_like(o["x"]))
        oo["x"][live] = o["x"][live]
        y, ref = _run_dense(wimg, n, oo, ("bias", "r1", "r2"))
        dead = torch.ones(n, dtype=torch.bool)
        dead[live] = False
        assert torch.equal(y[dead.to(DEV)], rest[dead.to(DEV)]), name
        _judge(name, y, W, oo["x"], **ref)


@pytest.mark.parametrize("n", [130, WALK2])
def test_nan_and_inf_stay_in_their_rows(layer, n):
    """One row holds a NaN, another an inf: those two output rows are non-finite and EVERY other row has the bits of the launch in which
    the two rows are zero -- the other 15 rows of the 16-row tile, the other 63 of the group, and (n = 16,485) the groups that the same
    workgroup stages next: the NaN sits in group 0 (workgroup 0 goes on to group 256), the inf in group 257 (staged by workgroup 1 while
    it works on group 1)."""
    W, wimg = layer
    o = _ops(n, seed=91)
    p_nan, p_inf = 5, n - 2
    assert p_inf // GROUP == (n - 1) // GROUP and p_nan // 16 != p_inf // 16
    clean = dict(o, x=o["x"].clone())
    clean["x"][[p_nan, p_inf]] = 0.0
    dirty = dict(o, x=clean["x"].clone())
    dirty["x"][p_nan] = o["x"][p_nan]
    dirty["x"][p_inf] = o["x"][p_inf]
    dirty["x"][p_nan, 77] = float("nan")
    dirty["x"][p_inf, 200] = float("inf")
    y0, ref = _run_dense(wimg, n, clean, ("bias", "r1"))
    y1, _ = _run_dense(wimg, n, dirty, ("bias", "r1"))
    assert not bool(torch.isfinite(y1[p_nan]).any()) and not bool(torch.isfinite(y1[p_inf]).any())
    others = torch.ones(n, dtype=torch.bool, device=DEV)
    others[[p_nan, p_inf]] = False
    differ = (y1 != y0).any(dim=1) & others
    assert not bool(differ.any()), torch.nonzero(differ).flatten()[:8].tolist()
    assert bool(torch.isfinite(y0).all())
    if n <= 200:
        _judge("nan_inf_clean_launch", y0, W, clean["x"], **ref)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the persistent walk
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walk_ops():
    return _ops(WALK3, seed=101)


@pytest.mark.parametrize("n", [WALK2, WALK3])
def test_walk_post0_with_r1(layer, walk_ops, n):
    """More groups than workgroups (the grid is capped at 256): every row meets its bound, and rows [0, 16384) have the bits of the
    16,384-row launch on the same buffers -- a row's result does not depend on how many groups its workgroup walks."""
    W, wimg = layer
    x, r1 = walk_ops["x"][:n].to(DEV), walk_ops["r1"][:n].to(DEV)
    y, y_short = torch.full((n, 256), 7.0, device=DEV), torch.full((n, 256), 7.0, device=DEV)
    _ws(wimg, n, (x, 256, 0), (y, 256, 0), r1=(r1, 256, 0))
    _ws(wimg, 16384, (x, 256, 0), (y_short, 256, 0), r1=(r1, 256, 0))
    _judge(f"walk_post0_{n}", y, W, walk_ops["x"][:n], r1=walk_ops["r1"][:n])
    assert torch.equal(y[:16384], y_short[:16384])
    assert _still_seven(y_short[16384:])


@pytest.mark.parametrize("n", [WALK2, WALK3])
def test_walk_post3_in_place_at_pitch_513(layer, walk_ops, n):
    """The dx accumulation of the backward chain over a walk: post 3 (relu'), r1 = x and r2 = y = dx at pitch 513 offset 257."""
    W, wimg = layer
    o = {k: walk_ops[k][:n] for k in ("x", "r1", "r2")}
    o["r1"] = o["r1"].clone()
    o["r1"].view(-1)[0::5] = 0.0
    xb = _place(o["x"], 256, 0)
    r1b = _place(o["r1"], 513, 257, seed=11)
    dx0 = _place(o["r2"], 513, 257, seed=12)[0]
    dx, dx_short = dx0.clone(), dx0.clone()
    _ws(wimg, n, xb, (dx, 513, 257), r1=r1b, r2=(dx, 513, 257), post=3, slope=0.0)
    _ws(wimg, 16384, xb, (dx_short, 513, 257), r1=r1b, r2=(dx_short, 513, 257), post=3, slope=0.0)
    _judge(f"walk_post3_{n}", dx[:, 257:], W, o["x"], r1=o["r1"], r2=o["r2"], post=3, slope=0.0)
    assert torch.equal(dx[:16384], dx_short[:16384])
    assert torch.equal(dx_short[16384:], dx0[16384:])                           # the short launch stops at its last row
    assert torch.equal(dx[:, :257], dx0[:, :257])


# ---------------------------------------------------------------------------------------------------------------------
# 5. amax_out
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [130, WALK2])
@pytest.mark.parametrize("post", [0, 2, 3])
def test_amax_out_is_the_maximum_of_what_was_written(layer, post, n):
    """A zeroed amax buffer receives exactly max |y[:n_rows, block]|; the rows behind n_rows of taller x / r1 / r2 buffers hold 1e6 and
    must not contribute (lanes past the end compute on a clamped row but neither store nor count)."""
    W, wimg = layer
    o = _ops(n, seed=111 + post)
    tall = 70
    xb = _place(o["x"], 256, 0, tall=tall, tall_value=1e6)
    r1b = _place(o["r1"], 513, 257, tall=tall, tall_value=1e6, seed=13)
    r2b = _place(o["r2"], 301, 3, tall=tall, tall_value=-1e6, seed=14)
    y = torch.full((n + tall, 301), 7.0, device=DEV)
    am = torch.zeros(_lib.AMAX_FLOATS, device=DEV)
    _ws(wimg, n, xb, (y, 301, 45), r1=r1b, r2=r2b, post=post, slope=0.2, w_fuse=0.7, amax_out=am)
    want = float(y[:n, 45:301].abs().max())
    assert float(am.max()) == want and want < 1e3
    assert _still_seven(y[n:]) and _still_seven(y[:, :45])
    record("ws_linear_amax_out", post=post, rows=n, amax=want)


# ---------------------------------------------------------------------------------------------------------------------
# 6. e3dge_ws_pack / e3dge_ws_image_bytes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", [None, (1e-4, 1e2)], ids=["randn", "1e-4_to_1e2"])
def test_pack_one_product_per_output(span):
    """x = 64 I (256 one-hot rows): output [k, f] is the single product 64 W[f, k], so the launch reads the packed image back.  split2
    keeps hi + lo = 11 + 11 bits (round toward zero, the remainder's exponent is at least 11 below the value's): 2^-21 |W| per entry.
    64 is a power of two, the row scale and its inverse are powers of two, and nothing else is summed, so no other rounding enters.
    The image stores lo 2^10 times too large (the kernel scales its partner down), so lo is a normal f16 down to |W| = 2^-20; with a
    plain lo the entries below 2^-10 kept only 2^-31 absolute -- 227 of these randn weights and 6,037 of the 1e-4 .. 1e+2 ones missed the
    bound, by up to 2^-14.1 of the entry."""
    lib = _lib.load()
    assert lib.e3dge_ws_image_bytes(1) == 8 * 8 * 2 * 2 * 64 * 16 == 2 * 2 * 256 * 256 and lib.e3dge_ws_image_bytes(3) == 3 * lib.e3dge_ws_image_bytes(1)
    W = _weights(17, span)
    wimg = _ws_image(W.to(DEV))
    assert wimg.numel() == lib.e3dge_ws_image_bytes(1)
    x = (64.0 * torch.eye(256)).to(DEV)
    y = torch.empty(256, 256, device=DEV)
    _ws(wimg, 256, (x, 256, 0), (y, 256, 0))
    w = W.double().t().abs()
    d = (y.cpu().double() - 64.0 * W.double().t()).abs() / 64.0                # |hi + lo - W| per entry
    worst = float((d / w).max())
    over = d > 2.0 ** -21 * w
    n_over, w_over = int(over.sum()), float(w[over].max()) if bool(over.any()) else 0.0
    record("ws_pack_onehot", span=str(span), worst_rel_log2=float(np.log2(max(worst, 1e-300))), worst_abs_log2=float(np.log2(max(float(d.max()), 1e-300))),
           entries_over=n_over, largest_w_over=w_over)
    print(f"ws_pack {span}: worst rel 2^{np.log2(max(worst, 1e-300)):.2f}, {n_over} entries over 2^-21 |W|, the largest of them |W| = {w_over:.3e}")
    assert n_over == 0, (n_over, worst, w_over)


# ---------------------------------------------------------------------------------------------------------------------
# 7. e3dge_ws_rowdot2
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 8193])
def test_rowdot2(n, gated):
    """out[row, 256] = a[row] . u + [gate > 0] b[row] . v into column 256 of a 513-wide buffer (8,193 rows: more than 4 x 2,048 blocks'
    worth, the grid-stride loop runs); +0, -0 and negative gates close, the smallest normal number opens.  Bound 1e-6 (|a| . |u| + |b| . |v|)
    per row; every other column and the rows behind the last keep their 7.0."""
    a, b, u, v = _randn(1, n, 256), _randn(2, n, 256), _randn(3, 256), _randn(4, 256)
    gate = None
    if gated:
        vals = torch.tensor([0.0, -0.0, -1.5, 2.0 ** -126, 1.0, 1e-30, -1e-30])
        gate = vals[torch.randint(0, len(vals), (n,), generator=torch.Generator().manual_seed(5))]
        if n >= 5:
            gate[:5] = vals[:5]
    out = torch.full((n + 3, 513), 7.0, device=DEV)
    gb = _place(gate[:, None], 513, 256, seed=21) if gated else (None, 0, 0)
    ag, ug, bg, vg = (t.to(DEV) for t in (a, u, b, v))
    _lib.launch("e3dge_ws_rowdot2", out, 513, 256, ag, ug, bg, vg, gb[0], gb[1], gb[2], n)
    sa, sb = a.double() @ u.double(), b.double() @ v.double()
    ref = sa + (sb * (gate > 0).double() if gated else sb)
    bound = 1e-6 * (a.double().abs() @ u.double().abs() + b.double().abs() @ v.double().abs())
    err = (out[:n, 256].cpu().double() - ref).abs()
    record("ws_rowdot2", rows=n, gated=gated, worst_err_over_bound=float((err / bound).max()) * 1e-6)
    assert bool((err <= bound).all()), (float((err / bound).max()), int(torch.argmax(err / bound)))
    assert _still_seven(out[:, :256]) and _still_seven(out[:, 257:])
    assert _still_seven(out[n:])


# ---------------------------------------------------------------------------------------------------------------------
# 8. e3dge_amax / e3dge_amax_rows
# ---------------------------------------------------------------------------------------------------------------------
def _amax(x, n):
    buf = torch.zeros(_lib.AMAX_FLOATS, device=DEV)
    _lib.launch("e3dge_amax", buf, x, n)
    return float(buf.max())


AMAX_BIG = 16 * 256 * 2048 + 13        # the grid cap (2,048 blocks) engages and the four-load trip runs


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4103, 65536 + 1, AMAX_BIG])
def test_amax_exact_wherever_the_maximum_sits(n):
    """max |x| must be exact (operand scales are derived from it).  |x| <= 1 everywhere but one planted -3.5, which is put in turn into
    the first element, the last full 16-byte vector, the scalar tail, and on both sides of the seams of the kernel's loops: between the
    loads of the four-load trip and between that trip and the single-load loop (elements 4 k stride +- 1, stride = 256 x blocks)."""
    x = torch.rand(n + 5, device=DEV, generator=torch.Generator(DEV).manual_seed(n)) * 2 - 1
    x[n:] = 9.0                                                                  # behind the end: must not be seen
    assert _amax(x, n) == float(x[:n].abs().max())
    blocks = min(max((n // 16 + 255) // 256, 1), 2048)
    stride = 256 * blocks
    spots = {0, n - 1, 4 * (n // 4) - 1, 4 * (n // 4) - 4, 4 * (n // 4)}
    for k in (1, 2, 3, 4, 5):
        spots |= {4 * k * stride - 1, 4 * k * stride, 4 * k * stride + 1}
    if n == AMAX_BIG:
        assert 4 * 4 * stride + 1 < 4 * (n // 4) < n                               # trip, single-load loop and tail all run
    for i in sorted(s for s in spots if 0 <= s < n):
        keep = float(x[i])
        x[i] = -3.5
        got = _amax(x, n)
        x[i] = keep
        assert got == 3.5, (n, i, got)


def test_amax_of_zeros_is_zero():
    for n in (5, 4103):
        assert _amax(torch.zeros(n, device=DEV), n) == 0.0
        assert _amax(-torch.zeros(n, device=DEV), n) == 0.0


@pytest.mark.parametrize("rows", [1, 7, 8, 9, 4096 * 8 + 5])
@pytest.mark.parametrize("width,ld", [(256, 301), (256, 513), (301, 301), (513, 513)])
def test_amax_rows_exact_and_blind_to_the_other_columns(rows, width, ld):
    """The same over the first `width` columns of rows of pitch `ld`: exact, the 9.0 in columns [width, ld) of every row and in the
    rows behind the last is not seen; a planted -3.5 is found in the first and the last element and (32,773 rows: the grid cap engages,
    the eight-load trip runs and the single-load loop takes the rest) on both sides of the seam between the two loops."""
    x = torch.rand(rows + 2, ld, device=DEV, generator=torch.Generator(DEV).manual_seed(rows + ld)) * 2 - 1
    x[:, width:] = 9.0
    x[rows:] = 9.0

    def run():
        buf = torch.zeros(_lib.AMAX_FLOATS, device=DEV)
        _lib.launch("e3dge_amax_rows", buf, x, rows, width, ld)
        return float(buf.max())
    assert run() == float(x[:rows, :width].abs().max()) <= 1.0
    n = rows * width
    blocks = min((n + 2047) // 2048, 4096)
    stride = 256 * blocks
    spots = {0, n - 1, width - 1, n - width} | {8 * stride * k + d for k in (1, 2) for d in (-1, 0, 1)}
    for e in sorted(s for s in spots if 0 <= s < n):
        r, c = divmod(e, width)
        keep = float(x[r, c])
        x[r, c] = -3.5
        got = run()
        x[r, c] = keep
        assert got == 3.5, (rows, width, ld, e, got)
