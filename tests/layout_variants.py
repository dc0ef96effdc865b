"""Layouts a caller may hand a module: `variant(x, kind)` is `torch.equal` to a dense tensor and has the stated property.  Pure torch,
CPU or GPU.  Every variant is a view into a larger buffer filled with SENTINEL; `Variant.check_untouched()` asserts afterwards that
neither the view nor one sentinel element changed (a kernel that wrote through an input, or past it).

    offset4        contiguous, data_ptr() % 16 == 4  (4-byte dtypes)
    pitch          unit last stride, rows padded by PITCH_PAD elements
    channels_last  4-D, stored (B, H, W, C)
    permuted       stored in another dimension order and permuted back: (B, D, N) storage for (B, N, D) points, the transpose for 2-D.
                   (For 4-D images the other order is NHWC, which is `channels_last`: the same strides, so it is not listed twice.)
    wide           a channel slice big[:, 1:1 + C] of a tensor with C + 2 channels
    expanded       x[:1].expand(B, ...): stride 0 over the first axis; its dense twin is x[:1].repeat(B, ...), not x
    expanded1      the same over the second axis, x[:, :1].expand(-1, n, ...): `latent.unsqueeze(1).expand(-1, n, -1)` styles.  Asked for
                   by name; `kinds_for` does not list it.
"""
import torch

SENTINEL = -777.25
PITCH_PAD = 3
GUARD = 4            # sentinel elements in front of a flat buffer: 16 bytes of float32, so the view keeps the buffer's alignment
KINDS = ("offset4", "pitch", "channels_last", "permuted", "wide", "expanded")


def _carve(x_shape, kind, make):
    """(buffer, view of shape x_shape): `make(shape)` allocates the buffer; the same carving serves the data and a bool mask of it."""
    shape = tuple(x_shape)
    n = 1
    for s in shape:
        n *= s
    if kind == "offset4":
        buf = make((n + 2 * GUARD,))
        return buf, buf[1:1 + n].view(shape)
    if kind == "pitch":
        buf = make(shape[:-1] + (shape[-1] + PITCH_PAD,))
        return buf, buf[..., :shape[-1]]
    if kind == "channels_last":
        B, C, H, W = shape
        buf = make((n + 2 * GUARD,))
        return buf, buf[GUARD:GUARD + n].view(B, H, W, C).permute(0, 3, 1, 2)
    if kind == "permuted":
        buf = make((n + 2 * GUARD,))
        if len(shape) == 3:
            B, N, D = shape
            return buf, buf[GUARD:GUARD + n].view(B, D, N).permute(0, 2, 1)
        N, D = shape
        return buf, buf[GUARD:GUARD + n].view(D, N).t()
    if kind == "wide":
        buf = make((shape[0], shape[1] + 2) + shape[2:])
        return buf, buf[:, 1:1 + shape[1]]
    if kind == "expanded":
        m = n // shape[0]
        buf = make((m + 2 * GUARD,))
        return buf, buf[GUARD:GUARD + m].view((1,) + shape[1:]).expand(shape)
    if kind == "expanded1":
        m = n // shape[1]
        buf = make((m + 2 * GUARD,))
        return buf, buf[GUARD:GUARD + m].view((shape[0], 1) + shape[2:]).expand(shape)
    raise ValueError(f"unknown layout kind {kind!r}")


def applies(x, kind):
    """Whether `kind` gives a tensor of x's shape a layout that differs from the dense one."""
    s = tuple(x.shape)
    if x.numel() == 0 or x.ndim == 0:
        return False
    if kind == "offset4":
        return x.element_size() == 4
    if kind == "pitch":
        return x.ndim >= 2 and x.numel() > s[-1]
    if kind == "channels_last":
        return x.ndim == 4 and s[1] > 1 and s[2] * s[3] > 1
    if kind == "permuted":
        return x.ndim in (2, 3) and s[-1] > 1 and s[-2] > 1
    if kind == "wide":
        return x.ndim >= 2          # (batch 1: still contiguous, but it starts one channel into the buffer)
    if kind == "expanded":
        return s[0] > 1
    if kind == "expanded1":
        return x.ndim >= 2 and s[1] > 1
    raise ValueError(f"unknown layout kind {kind!r}")


def kinds_for(x):
    return [k for k in KINDS if applies(x, k)]


def dense_twin(x, kind):
    """The dense tensor `variant(x, kind)` is equal to: x, or for `expanded` the first slice repeated."""
    if kind == "expanded":
        return x[:1].repeat((x.shape[0],) + (1,) * (x.ndim - 1)).contiguous()
    if kind == "expanded1":
        return x[:, :1].repeat((1, x.shape[1]) + (1,) * (x.ndim - 2)).contiguous()
    return x.contiguous()


class Variant:
    """`.tensor` is the view, `.buffer` what surrounds it, `.mask` True where the buffer holds the view's elements."""

    def __init__(self, x, kind):
        if not applies(x, kind):
            raise ValueError(f"layout {kind!r} does not apply to a tensor of shape {tuple(x.shape)}")
        fill = SENTINEL if x.is_floating_point() else -7
        self.kind = kind
        self.buffer, view = _carve(x.shape, kind, lambda shape: torch.full(shape, fill, device=x.device, dtype=x.dtype))
        if kind == "expanded":
            view[:1].copy_(x[:1])
        elif kind == "expanded1":
            view[:, :1].copy_(x[:, :1])
        else:
            view.copy_(x)
        self.mask, mview = _carve(x.shape, kind, lambda shape: torch.zeros(shape, device=x.device, dtype=torch.bool))
        if kind == "expanded":
            mview[:1].fill_(True)
        elif kind == "expanded1":
            mview[:, :1].fill_(True)
        else:
            mview.fill_(True)
        self.tensor = view
        self.snapshot = self.buffer.clone()

    def check_untouched(self):
        assert torch.equal(self.buffer, self.snapshot), f"the {self.kind} input or the sentinels around it were written"


def variant(x, kind):
    return Variant(x, kind).tensor
