"""GPU: the fp32-MFMA implicit-GEMM convolutions of LPIPS, the identity term and the discriminator (csrc/conv_igemm.h and the four kernels
built on it) must stay BIT-identical across changes that only move code.  Accumulation order is what the repeatability and
batch-independence tests rest on, so every output is compared with the recording made on the MI355X from the commit before the kernels
shared one core: small outputs element by element, large ones and the packed weight images by SHA-256 of their bytes.

Tile width: NT = tile_width(pixels, images counted, channel blocks) below restates the library's rule; every case asserts the NT it is meant
to run, so a changed rule fails here instead of quietly testing NT = 1 three times.

Single-layer sweep (n = 2, 8 -> 64 channels: one 64-channel block), kernel 1 and 3, stride 1 and 2, GEMM pixel planes 9x11 / 64x64 / 96x96
= NT 1 / 2 / 4, sized by the output plane under stride 2; K = 8 and 72 (forward) or 64 and 576 (gradient):
    idnet/...     e3dge_idnet_conv, input affine + epilogue affine + PReLU + plane sums  idnet_conv_kernel<KS, STRIDE, NT> and conv_pack_kernel
    idnet_bwd/... e3dge_idnet_conv_bwd, `a`: per-image in_ab + mask / slope + addend (stride 1), `b`: scale + addend
                                                                                      idnet_dgrad_kernel<KS, STRIDE, NT> and conv_pack_t_kernel
                  (the C entry reads its addend with stride 1; the stride-2 addend and in_scale run in the whole network: units 0, 3, 7, 21)
    disc/...      e3dge_disc_conv, `a`: bias + lrelu + merged addend, `b`: added addend  disc_gemm_kernel<KS, 0 / 1, NT> and conv_pack_kernel
    disc_bwd/...  e3dge_disc_conv_dgrad, `a`: sign with s_pos / s_neg + addend, `b`: one factor
                                                                                      disc_gemm_kernel<KS, 0 / 2, NT> and conv_pack_t_kernel
  ragged K:       idnet 3 -> 64 at 9x11 (K = 27, and the M = 3 gradient with one live wave), disc 3 -> 64 1x1 at 16^2 (K = 3) and 513 -> 512
                  at 4^2 (K = 4617 forward, M = 513 gradient: a ragged last channel tile), all NT = 1.
Whole networks, synthetic weights, forward and backward through the Python modules:
    lpips/small   1 pair 67x71: NT = 1 at all five convolutions and four data gradients
    lpips/large   1 pair 380x380: conv 1 runs lpips_conv_kernel<11, 4, 2, 4, true> (N = 2 * 94^2 = 17672), conv 2 <5, 1, 2, 2, false>
                  (N = 4232, 3 blocks), conv 3 to 5 and all four data gradients (N = 968 and 4232 with 6, 4, 3 and 1 blocks) NT = 1
    idloss/n1     1 pair 256^2, saving forward + backward: idnet_conv_kernel<3, 1, NT, true>, <3, 1 / 2, NT> and <1, 2, NT>: NT = 4 at
                  112^2, NT = 2 for 128 channels at 56^2, NT = 1 everywhere else (64 channels at 56^2 and all of 28^2, 14^2, 7^2);
                  idnet_dgrad_kernel<3, 1 / 2, NT> and <1, 2, NT>: NT = 4 at 112^2 (the M = 3 gradient and the stride-2 addend of unit 0
                  included), NT = 2 for 128 channels at 56^2, else NT = 1
    disc/init64   init_size 64, batch 2, saving forward + backward: disc_gemm_kernel NT = 4 at 64^2 and 32^2, NT = 2 for the M = 3 stem
                  gradient, NT = 1 from 16^2 down

Record the fixture (on the GPU, from the commit whose numerics are the yardstick):
    python tests/test_gpu_conv_bitexact.py --record"""
import functools
import hashlib
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from conftest import GOLDEN  # noqa: E402

import e3dge_amd  # noqa: E402,F401
from e3dge_amd import _lib, synthetic as syn  # noqa: E402
from e3dge_amd.discriminator import Discriminator  # noqa: E402
from e3dge_amd.id_loss import IDLoss  # noqa: E402
from e3dge_amd.lpips import LPIPS  # noqa: E402
from test_discriminator_host import golden_images as disc_images  # noqa: E402
from test_idloss_host import golden_images as id_images, make_pair  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = os.path.join(GOLDEN, "conv_bitexact.npz")
RAW_BYTES = 256                                                      # larger outputs are stored as digests
SQRT2 = 2 ** 0.5


def tile_width(pixels, images, gy):
    """The library's rule: the widest tile of 16 NT pixels that still gives each of the 256 CUs a workgroup for `images` images."""
    blocks = lambda bn: (pixels + bn - 1) // bn
    return 4 if blocks(64) * images * gy >= 256 else 2 if blocks(32) * images * gy >= 256 else 1


def keep(out, name, t):
    """Store tensor t under `name`: raw when small, else the SHA-256 of its bytes."""
    a = t.detach().contiguous().cpu().numpy()
    if a.nbytes <= RAW_BYTES:
        out[name] = a
    else:
        out[name + "_sha256"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy()


def kpad(c, k):
    return (c * k * k + 31) // 32 * 32


def mpad(m):
    return (m + 15) // 16 * 16


# ---- single layers ----------------------------------------------------------------------------------------------------------------
PLANES = [((9, 11), 1), ((64, 64), 2), ((96, 96), 4)]                # the GEMM's pixel plane and the NT it must get
SWEEP = [(2, 8, 64, plane, k, s, nt) for k in (1, 3) for s in (1, 2) for plane, nt in PLANES]
RAGGED_ID = [(2, 3, 64, (9, 11), 3, 1, 1)]
RAGGED_DC = [(3, 3, 64, (16, 16), 1, 1, 1), (3, 513, 512, (4, 4), 3, 1, 1)]


def case_name(c):
    n, ci, co, (ph, pw), k, s, nt = c
    return f"{n}x{ci}x{co}_{ph}x{pw}_k{k}s{s}"


def normal(rs, *shape, scale=1.0, shift=0.0):
    return torch.from_numpy(shift + scale * rs.standard_normal(shape)).float().to(DEV)


def idnet_layer(out, c, seed):
    n, ci, co, (OH, OW), k, s, nt = c
    lib = _lib.load()
    assert tile_width(OH * OW, 2, co // 64) == nt, c
    H, W = (OH, OW) if s == 1 else (2 * OH - 1, 2 * OW - 1)
    tiles = lib.e3dge_idnet_conv_tiles(co, H, W, k, s)
    assert tiles == (OH * OW + 16 * nt - 1) // (16 * nt), (c, tiles)
    rs = np.random.RandomState(seed)
    x, w = normal(rs, n, ci, H, W), normal(rs, co, ci, k, k, scale=(2.0 / (ci * k * k)) ** 0.5)
    in_ab = torch.stack([normal(rs, ci, scale=0.2, shift=1.0), normal(rs, ci, scale=0.5, shift=0.3)], 1).contiguous()
    epi_ab = torch.stack([normal(rs, co, scale=0.2, shift=1.0), normal(rs, co, scale=0.5)], 1).contiguous()
    slope = normal(rs, co, scale=0.05, shift=0.25)
    y = torch.zeros(n, co, OH, OW, device=DEV)
    part = torch.zeros(n, co, tiles, device=DEV)
    wfrag = torch.zeros(co * kpad(ci, k), device=DEV)
    _lib.launch("e3dge_idnet_conv", y, x, w, wfrag, in_ab, epi_ab, slope, part, n, ci, co, H, W, k, s)
    key = "idnet/" + case_name(c)
    keep(out, key + "/out", y), keep(out, key + "/plane", part), keep(out, key + "/wfrag", wfrag)


def idnet_dgrad_layer(out, c, seed):
    n, ci, co, (H, W), k, s, nt = c
    assert tile_width(H * W, 2, (ci + 63) // 64) == nt, c
    GH, GW = (H - 1) // s + 1, (W - 1) // s + 1
    rs = np.random.RandomState(seed)
    g, w = normal(rs, n, co, GH, GW), normal(rs, co, ci, k, k, scale=(2.0 / (ci * k * k)) ** 0.5)
    in_ab = torch.stack([normal(rs, n, co, scale=0.2, shift=1.0), normal(rs, n, co, scale=0.5, shift=0.3)], 2).contiguous()
    mask = torch.from_numpy(rs.randint(0, 2, size=(n, ci, H, W)).astype(np.uint8)).to(DEV)
    slope, scale, addend = normal(rs, ci, scale=0.3, shift=0.05), normal(rs, ci, scale=0.2, shift=1.0), normal(rs, n, ci, H, W)
    key = "idnet_bwd/" + case_name(c)
    for v, (ab, m, sl, sc) in (("a", (in_ab, mask, slope, None)), ("b", (None, None, None, scale))):
        y = torch.zeros(n, ci, H, W, device=DEV)
        wfrag_t = torch.zeros(mpad(ci) * kpad(co, k), device=DEV)
        _lib.launch("e3dge_idnet_conv_bwd", y, g, w, wfrag_t, ab, m, sl, sc, addend, n, ci, co, H, W, k, s)
        keep(out, f"{key}/{v}/out", y)
    keep(out, key + "/wfrag_t", wfrag_t)


def disc_layer(out, c, seed):
    n, ci, co, (OH, OW), k, s, nt = c
    assert tile_width(OH * OW, 2, (co + 63) // 64) == nt, c
    H, W = (OH, OW) if s == 1 else (2 * (OH - 1) + k, 2 * (OW - 1) + k)
    rs = np.random.RandomState(seed)
    x, w, bias, addend = normal(rs, n, ci, H, W), normal(rs, co, ci, k, k), normal(rs, co, scale=0.5), normal(rs, n, co, OH, OW)
    scale = 1 / math.sqrt(ci * k * k)
    key = "disc/" + case_name(c)
    for v, (b, act, merge) in (("a", (bias, 1, 1)), ("b", (None, 0, 0))):
        y = torch.zeros(n, co, OH, OW, device=DEV)
        wfrag = torch.zeros(mpad(co) * kpad(ci, k), device=DEV)
        _lib.launch("e3dge_disc_conv", y, x, w, wfrag, b, addend, n, ci, co, H, W, k, s, act, merge, float(scale))
        keep(out, f"{key}/{v}/out", y)
    keep(out, key + "/wfrag", wfrag)


def disc_dgrad_layer(out, c, seed):
    n, ci, co, (H, W), k, s, nt = c
    assert tile_width(H * W, 2, (ci + 63) // 64) == nt, c
    GH, GW = (H, W) if s == 1 else ((H - k) // 2 + 1, (W - k) // 2 + 1)
    rs = np.random.RandomState(seed)
    g, w, sign, addend = normal(rs, n, co, GH, GW), normal(rs, co, ci, k, k), normal(rs, n, co, GH, GW), normal(rs, n, ci, H, W)
    scale = 1 / math.sqrt(ci * k * k)
    key = "disc_bwd/" + case_name(c)
    for v, (sg, s_pos, s_neg, add) in (("a", (sign, SQRT2, 0.2 * SQRT2, addend)), ("b", (None, 1 / SQRT2, 1 / SQRT2, None))):
        y = torch.zeros(n, ci, H, W, device=DEV)
        wfrag_t = torch.zeros(mpad(ci) * kpad(co, k), device=DEV)
        _lib.launch("e3dge_disc_conv_dgrad", y, g, w, wfrag_t, sg, float(s_pos), float(s_neg), add, n, ci, co, H, W, k, s, float(scale))
        keep(out, f"{key}/{v}/out", y)
    keep(out, key + "/wfrag_t", wfrag_t)


def layers():
    out = {}
    for i, c in enumerate(SWEEP + RAGGED_ID):
        idnet_layer(out, c, 400 + i)
        idnet_dgrad_layer(out, c, 500 + i)
    for i, c in enumerate(SWEEP + RAGGED_DC):
        disc_layer(out, c, 600 + i)
        disc_dgrad_layer(out, c, 700 + i)
    torch.cuda.synchronize()
    return out


# ---- whole networks ---------------------------------------------------------------------------------------------------------------
def lpips_net(out, name, shape, nts):
    B, _, H, W = shape
    h0, w0 = (H + 4 - 11) // 4 + 1, (W + 4 - 11) // 4 + 1
    h1, w1 = (h0 - 3) // 2 + 1, (w0 - 3) // 2 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    got = [tile_width(2 * B * hw, 1, gy) for hw, gy in ((h0 * w0, 1), (h1 * w1, 3), (h2 * w2, 6), (h2 * w2, 4), (h2 * w2, 4))]
    got += [tile_width(2 * B * hw, 1, gy) for hw, gy in ((h2 * w2, 4), (h2 * w2, 6), (h2 * w2, 3), (h1 * w1, 1))]   # the gradients of conv 5 .. 2
    assert got == nts, (name, got)
    m = syn.load_synthetic_lpips(LPIPS()).to(DEV)
    x, y = (t.to(DEV) for t in make_pair(shape, seed=sum(shape)))
    with torch.no_grad():
        r = m.run(x, y, per_layer=True)
    gx, gy, _ = m.run_backward(x, y, torch.linspace(0.5, 1.5, B).to(DEV) if B > 1 else torch.ones(1, device=DEV), want_x=True, want_y=True)
    key = "lpips/" + name
    keep(out, key + "/per_image", r['per_image']), keep(out, key + "/per_layer", r['per_layer'])
    keep(out, key + "/grad_x", gx), keep(out, key + "/grad_y", gy)


def idloss_net(out):
    for pix, gy, nt in ((112 * 112, 1, 4), (56 * 56, 1, 1), (56 * 56, 2, 2), (28 * 28, 2, 1), (28 * 28, 4, 1), (14 * 14, 8, 1), (7 * 7, 8, 1)):
        assert tile_width(pix, 2, gy) == nt, (pix, gy)               # (pixels, 64-channel blocks): the NT the docstring lists
    m = syn.load_synthetic_idloss(IDLoss()).to(DEV)
    pred, gt = (t.to(DEV) for t in id_images(1, 256))
    with torch.no_grad():
        r = m.run(pred, gt)
    grad = m.run_backward(pred, gt, torch.ones(1, device=DEV))[0]
    keep(out, "idloss/n1/embeddings", r['embeddings']), keep(out, "idloss/n1/dots", r['dots']), keep(out, "idloss/n1/grad", grad)


def disc_net(out):
    for pix, M, nt in ((64 * 64, 256, 4), (32 * 32, 512, 4), (64 * 64, 3, 2), (16 * 16, 512, 1)):
        assert tile_width(pix, 2, (M + 63) // 64) == nt, (pix, M)
    m = syn.load_synthetic_discriminator(Discriminator(syn.discriminator_opt(64, 1))).to(DEV)
    for p in m.parameters():
        p.requires_grad_(False)
    x = disc_images(2, 64).to(DEV)
    r = m.run_backward(x, torch.tensor([[0.25], [0.75]], device=DEV))
    keep(out, "disc/init64/logits", r['logits']), keep(out, "disc/init64/grad", r['grad'])


def networks():
    out = {}
    lpips_net(out, "small", (1, 3, 67, 71), [1] * 9)
    lpips_net(out, "large", (1, 3, 380, 380), [4, 2, 1, 1, 1, 1, 1, 1, 1])
    idloss_net(out)
    disc_net(out)
    torch.cuda.synchronize()
    return out


GROUPS = {"layers": layers, "networks": networks}


@functools.lru_cache(maxsize=None)
def computed(group):
    return GROUPS[group]()


def save_fixture(path, res):
    """One (names, 32-byte rows) table for the digests, the small outputs as arrays of their own."""
    names = sorted(k for k in res if k.endswith("_sha256"))
    np.savez_compressed(path, digest_names=np.array(names), digests=np.stack([res[k] for k in names]),
                        **{k: v for k, v in res.items() if k not in names})


def load_fixture(path):
    f = np.load(path)
    ref = {k: f[k] for k in f.files if k not in ("digest_names", "digests")}
    ref.update(zip(f["digest_names"].tolist(), f["digests"]))
    return ref


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_conv_outputs_bit_identical(group):
    if not os.path.exists(FIXTURE):
        pytest.fail("bit-identity fixture missing (record it: python tests/test_gpu_conv_bitexact.py --record)")
    ref = {k[len(group) + 1:]: v for k, v in load_fixture(FIXTURE).items() if k.startswith(group + ":")}
    got = computed(group)
    assert set(ref) == set(got), sorted(set(ref) ^ set(got))
    bad = [k for k in sorted(got) if got[k].dtype != ref[k].dtype or got[k].shape != ref[k].shape or got[k].tobytes() != ref[k].tobytes()]
    assert not bad, f"not bit-identical: {bad}"


def test_single_layers_are_deterministic():
    first, again = computed("layers"), layers()
    assert [k for k in first if first[k].tobytes() != again[k].tobytes()] == []


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_gpu_conv_bitexact.py --record")
    res = {group + ":" + k: v for group in GROUPS for k, v in computed(group).items()}
    save_fixture(FIXTURE, res)
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes,", len(res), "entries")
