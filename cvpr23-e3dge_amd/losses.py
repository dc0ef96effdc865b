"""The training loss that joins the HIP nodes: the counterpart of the reference's `project/losses/builder.py: LossClass`, the trainers'
`pool_256` / `pool_64` (trainer.py:1023-1025) and `gan_loss.eikonal_loss` (gan_loss.py:14-25), on the kernels of csrc/losses.hip.

    AvgPool2d(size)        AdaptiveAvgPool2d at an integer ratio: e3dge_avgpool_fwd / e3dge_avgpool_bwd
    eikonal_loss           the reference's function (plain torch; inside LossClass the term is one segment of the shape launch)
    g_nonsaturating_loss, d_logistic_loss, d_r1_loss
                           the reference's GAN terms (gan_loss.py:28-48, plain torch on the B logits of e3dge_amd.discriminator)
    LossClass              calc_shape_rec_loss: every enabled term in two forward launches and one backward launch
                           calc_2d_rec_loss:    MSE from e3dge_image_metrics' sums with e3dge_sqerr_bwd as its backward, LPIPS and the
                                                identity term through e3dge_amd.lpips.LPIPS / e3dge_amd.id_loss.IDLoss (differentiable)

GPU float32 tensors take the HIP kernels; CPU tensors, other dtypes, non-integer pool ratios and second-order gradients take the torch
formulas, which are the reference's own.  The loss nodes are once-differentiable; the eikonal term's double backward belongs to the
renderer node that produced it.  Out of scope, as in the reference's callers: the fg_mask products (the caller's, before the call),
ConsistencyLoss and DepthLoss; LossClass itself does not call the GAN terms (the trainer adds them, trainer.py:1233-1244)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .sharded_eval import image_metrics, image_metrics_torch

POOL_FACTORS = (1, 2, 4, 8, 16)
SHAPE_TERMS = ("sdf_rec_loss", "surf_rec_loss", "surface_norm_rec_loss", "eikonal_term")      # the reference's order of summation


def _is_hip(t):
    return torch.is_tensor(t) and t.device.type == "cuda" and t.dtype == torch.float32


# ---------------------------------------------------------------------------------------------------------------------- pool
class _AvgPoolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, f):
        shape = tuple(x.shape)
        H, W = shape[-2:]
        planes = x.numel() // (H * W)
        out = torch.empty(shape[:-2] + (H // f, W // f), device=x.device, dtype=torch.float32)
        _lib.launch("e3dge_avgpool_fwd", out, x, planes, H, W, f)
        ctx.shape, ctx.f = shape, f
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        f = ctx.f
        if torch.is_grad_enabled() or not _is_hip(g):     # create_graph=True: the (linear) torch expression, differentiable again
            return g.repeat_interleave(f, -2).repeat_interleave(f, -1) / (f * f), None
        H, W = ctx.shape[-2:]
        g = g.contiguous()
        d = torch.empty(ctx.shape, device=g.device, dtype=torch.float32)
        _lib.launch("e3dge_avgpool_bwd", d, g, d.numel() // (H * W), H, W, f)
        return d, None


class AvgPool2d(nn.Module):
    """`AvgPool2d((256, 256))`: a drop-in for the trainers' `pool_256` / `pool_64` (torch.nn.AdaptiveAvgPool2d).  GPU float32 contiguous
    inputs whose height and width are the same multiple f in {1, 2, 4, 8, 16} of the output's take the HIP kernels through one autograd
    Function (once-differentiable: a backward under create_graph=True runs the torch expression); everything else -- CPU tensors, other
    dtypes, strided inputs, any other ratio -- is F.adaptive_avg_pool2d."""

    def __init__(self, output_size):
        super().__init__()
        self.output_size = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)

    def factor(self, x):
        """The integer ratio the HIP kernels would pool `x` by, or None when `x` takes the torch branch."""
        if not _is_hip(x) or x.ndim not in (3, 4) or not x.is_contiguous() or x.numel() == 0 or None in self.output_size:
            return None
        (H, W), (oh, ow) = x.shape[-2:], self.output_size
        if oh < 1 or ow < 1 or H % oh or W % ow or H // oh != W // ow or H // oh not in POOL_FACTORS:
            return None
        return H // oh

    def forward(self, x):
        f = self.factor(x)
        if f is None:
            return F.adaptive_avg_pool2d(x, self.output_size)
        return _AvgPoolFunction.apply(x, f)

    def extra_repr(self):
        return f"output_size={self.output_size}"


# ------------------------------------------------------------------------------------------------------------------- eikonal
def eikonal_loss(eikonal_term, sdf=None, beta=100):
    """gan_loss.py:14-25: (mean((|e| - 1)^2), mean(exp(-beta |sdf|)) or a zero tensor).  Plain torch."""
    eik = 0 if eikonal_term is None else ((eikonal_term.norm(dim=-1) - 1) ** 2).mean()
    if sdf is None:
        minimal_surface = torch.tensor(0.0, device=eikonal_term.device)
    else:
        minimal_surface = torch.exp(-beta * torch.abs(sdf)).mean()
    return eik, minimal_surface


# ----------------------------------------------------------------------------------------------------------------- GAN terms
# gan_loss.py:28-48, plain torch: they act on the B logits of e3dge_amd.discriminator.Discriminator.
def d_logistic_loss(real_pred, fake_pred):
    return F.softplus(-real_pred).mean() + F.softplus(fake_pred).mean()


def d_r1_loss(real_pred, real_img):
    """The R1 penalty: a double backward through the discriminator, which therefore runs its torch composition (trainable parameters)."""
    grad_real, = torch.autograd.grad(outputs=real_pred.sum(), inputs=real_img, create_graph=True)
    return grad_real.pow(2).reshape(grad_real.shape[0], -1).sum(1).mean()


def g_nonsaturating_loss(fake_pred):
    return F.softplus(-fake_pred).mean()


# --------------------------------------------------------------------------------------------------------------- shape terms
def _shape_args(slots, device):
    """E3dgeShapeLossArgs for `slots`: four entries, None (off) or (kind, pred, gt or None, lambda)."""
    a = _lib.ShapeLossArgs()
    for i, slot in enumerate(slots):
        if slot is None:
            continue
        kind, pred, gt, lam = slot
        s = a.seg[i]
        s.kind, s.pred, s.gt, s.lambda_ = kind, pred, gt, float(lam)
        s.n = pred.numel() // 3 if kind == _lib.SHAPE_EIKONAL else pred.numel()
    a._note(device)
    return a


class _ShapeLossFunction(torch.autograd.Function):
    """(total, terms (4,)) of the enabled terms: one tile launch and one fold launch; the backward is one launch.  The graph leads to
    the predictions through `total` only."""

    @staticmethod
    def forward(ctx, kinds, lambdas, *tensors):
        preds, gts = tensors[:4], tensors[4:]
        dev = next(p for p in preds if p is not None).device
        slots = [None if p is None else (k, p.detach().contiguous(), None if g is None else g.detach().contiguous(), lam)
                 for k, lam, p, g in zip(kinds, lambdas, preds, gts)]
        a = _shape_args(slots, dev)
        n_partial = _lib.load().e3dge_shape_loss_partial_floats(a)
        out = torch.empty(5 + n_partial, device=dev, dtype=torch.float32)     # the fold writes all four terms and the total
        a.terms, a.total, a.partial, a.partial_floats = out.data_ptr(), out.data_ptr() + 16, out.data_ptr() + 20, n_partial
        _lib.launch("e3dge_shape_loss_fwd", a)
        ctx.slots, ctx.dev = slots, dev
        ctx.set_materialize_grads(False)
        total, terms = out[4], out[:4]
        ctx.mark_non_differentiable(terms)
        return total, terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_total, g_terms):
        grads = [None] * 8
        if g_total is None:
            return (None, None, *grads)
        want = [s is not None and ctx.needs_input_grad[2 + i] for i, s in enumerate(ctx.slots)]
        a = _shape_args([s if w else None for s, w in zip(ctx.slots, want)], ctx.dev)
        for i, s in enumerate(ctx.slots):
            if want[i]:
                grads[i] = torch.empty_like(s[1])
                a.seg[i].d_pred = grads[i]
        a.upstream = g_total.to(torch.float32).contiguous()
        _lib.launch("e3dge_shape_loss_bwd", a)
        return (None, None, *grads)


class _MseFunction(torch.autograd.Function):
    """mean((pred - gt)^2) as e3dge_image_metrics computes it (the per-image sums stay in `side` for the report columns); the backward
    is e3dge_sqerr_bwd with the upstream scale read from device memory."""

    @staticmethod
    def forward(ctx, pred, gt, side):
        B, C, H, W = pred.shape
        p, g = pred.detach().contiguous(), gt.detach().contiguous()
        sums = torch.empty((B, 4), device=p.device, dtype=torch.float32)
        scratch = torch.empty(_lib.load().e3dge_image_metrics_scratch_floats(B, C, H, W), device=p.device, dtype=torch.float32)
        _lib.launch("e3dge_image_metrics", sums, scratch, p, g, B, C, H, W, 1.0)
        row = torch.empty(8, device=p.device, dtype=torch.float32)
        _lib.launch("e3dge_image_metric_row", row, sums, None, None, B, 1.0, 0.0, 0.0)
        side['sums'], side['pred'], side['gt'] = sums, p, g
        ctx.save_for_backward(p, g)
        ctx.set_materialize_grads(False)
        return row[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_mse):
        if g_mse is None or not ctx.needs_input_grad[0]:
            return None, None, None
        p, g = ctx.saved_tensors
        scale = (g_mse.to(torch.float32) * (2.0 / p.numel())).contiguous()
        d = torch.empty_like(p)
        _lib.launch("e3dge_sqerr_bwd", d, p, g, p.numel(), scale)
        return d, None, None


# ----------------------------------------------------------------------------------------------------------------- LossClass
class LossClass(nn.Module):
    """`LossClass(device, opt)` with the reference's attributes and methods (builder.py:8-190).  `lpips` / `id_loss`: the modules to use
    as criterionLPIPS / criterionID (any callables on CPU tensors); the defaults are `e3dge_amd.lpips.LPIPS(differentiable=True)` and
    `e3dge_amd.id_loss.IDLoss(differentiable=True)` on `device`, whose weights come from local files only (their load_pretrained)."""

    def __init__(self, device, opt, lpips=None, id_loss=None):
        super().__init__()
        self.opt = opt
        self.device = device
        self.criterionImg = nn.MSELoss()
        if lpips is None:
            from .lpips import LPIPS
            lpips = LPIPS(device=device, net_type='alex', differentiable=True).eval()
        if id_loss is None:
            from .id_loss import IDLoss
            id_loss = IDLoss(device=device, differentiable=True).eval()
        self.criterionLPIPS = lpips
        self.criterionID = id_loss
        self.criterion3d_rec = nn.SmoothL1Loss()
        self.id_loss_pool = AvgPool2d((256, 256))
        self.uniform_pts_loss = nn.BCEWithLogitsLoss()

    def psnr_loss(self, input, target, max_val):
        return 10.0 * torch.log10(max_val ** 2 / torch.mean((input - target) ** 2))

    # ---- 3-D ----------------------------------------------------------------------------------------------------------------------
    def calc_shape_rec_loss(self, pred_shape, gt_shape, device, supervise_sdf=True, supervise_surface=False,
                            supervise_surface_normal=False, supervise_eikonal=False, supervise_chamfer_dist=False):
        """(shape_loss, dict of SHAPE_TERMS) of builder.py:43-117.  A term is skipped (its entry stays a zero tensor) when its flag is
        off or its lambda is <= 0.  GPU float32: one _ShapeLossFunction for all enabled terms; the dictionary entries are detached."""
        opt = self.opt
        assert supervise_sdf or supervise_surface_normal, 'should at least supervise one types of shape reconstruction'
        # the reference's zero defaults; one fill launch, where four torch.tensor(0., device=...) are four host-to-device copies
        out = dict(zip(("surf_rec_loss", "sdf_rec_loss", "surface_norm_rec_loss", "eikonal_term"), torch.zeros(4, device=device).unbind(0)))
        S, E = _lib.SHAPE_SMOOTH_L1, _lib.SHAPE_EIKONAL
        slots = [None] * 4                                            # (kind, pred, gt, lambda), in SHAPE_TERMS order
        if supervise_sdf and opt.uniform_pts_sdf_lambda > 0:
            slots[0] = (S, pred_shape['uniform_points_sdf'].squeeze(), gt_shape['uniform_points_sdf'].squeeze(), opt.uniform_pts_sdf_lambda)
        if supervise_surface and opt.surf_sdf_lambda > 0:
            slots[1] = (S, pred_shape['surface_sdf'], None, opt.surf_sdf_lambda)
        if supervise_surface_normal and opt.surf_normal_lambda > 0:
            slots[2] = (S, pred_shape['surface_eikonal_term'].squeeze(), gt_shape['surface_eikonal_term'].squeeze(), opt.surf_normal_lambda)
        if supervise_eikonal and opt.eikonal_lambda > 0:
            slots[3] = (E, pred_shape['eikonal_term'], None, opt.eikonal_lambda)
        live = [s for s in slots if s is not None]
        if not live:
            return 0, out
        if self._shape_on_hip(live):
            total, terms = _ShapeLossFunction.apply(tuple(S if s is None else s[0] for s in slots), tuple(0.0 if s is None else s[3] for s in slots),
                                                    *[None if s is None else s[1] for s in slots], *[None if s is None else s[2] for s in slots])
            for i, name in enumerate(SHAPE_TERMS):
                if slots[i] is not None:
                    out[name] = terms[i]
            return total, out
        shape_loss = 0
        for i, name in enumerate(SHAPE_TERMS):                        # the reference's formulas, in its order
            if slots[i] is None:
                continue
            kind, pred, gt, lam = slots[i]
            if kind == E:
                out[name] = eikonal_loss(pred)[0] * lam
            else:
                out[name] = self.criterion3d_rec(pred, torch.zeros_like(pred) if gt is None else gt) * lam
            shape_loss = shape_loss + out[name]
        return shape_loss, out

    @staticmethod
    def _shape_on_hip(live):
        dev = live[0][1].device
        for kind, pred, gt, _ in live:
            if not _is_hip(pred) or pred.device != dev or pred.numel() == 0:
                return False
            if gt is not None and (not _is_hip(gt) or gt.device != dev or gt.shape != pred.shape or (torch.is_grad_enabled() and gt.requires_grad)):
                return False
            if kind == _lib.SHAPE_EIKONAL and (pred.ndim < 1 or pred.shape[-1] != 3):
                return False
        return True

    # ---- 2-D ----------------------------------------------------------------------------------------------------------------------
    def calc_2d_rec_loss(self, rgb_images, rgb_gt, high_res_rgb_gt, opt, loss_dict=False, mode='train'):
        """builder.py:130-186: (loss, loss_l2, loss_lpips, loss_id, 0, 0), or (loss, dict of the eight columns) with loss_dict=True.
        loss = (l2_lambda MSE + vgg_lambda LPIPS) + id_lambda loss_id in float32, in that order."""
        opt = self.opt
        l2, vgg, idl = float(opt.l2_lambda), float(opt.vgg_lambda), float(opt.id_lambda)
        pred, gt = rgb_images, rgb_gt
        id_mod = self.criterionID if idl > 0 else None
        on_hip = _is_hip(pred) and _is_hip(gt) and pred.ndim == 4 and pred.shape == gt.shape and pred.device == gt.device
        if on_hip and torch.is_grad_enabled() and pred.requires_grad and not gt.requires_grad:
            side = {}
            mse = _MseFunction.apply(pred, gt, side)
            p, g = side['pred'], side['gt']
            if vgg != 0:
                lp_res = self.criterionLPIPS.run(pred, g)
            else:                                                     # the column only: no graph for a term of weight 0
                with torch.no_grad():
                    lp_res = self.criterionLPIPS.run(p, g)
            lp = lp_res['mean']
            lid = id_mod.run(pred, g)['loss'] if id_mod is not None else torch.zeros((), device=pred.device)
            loss = (mse * l2 + lp * vgg) + lid * idl
            row = torch.empty(8, device=pred.device, dtype=torch.float32)
            _lib.launch("e3dge_image_metric_row", row, side['sums'], lp_res['per_image'].detach(),
                        lid.detach() if id_mod is not None else None, pred.shape[0], l2, vgg, idl)
            cols = [mse, lid, lp, loss, row[4], row[5], row[6], row[7]]
        else:
            if on_hip and not (torch.is_grad_enabled() and gt.requires_grad):
                row = image_metrics(pred, gt, l2, self.criterionLPIPS, vgg, id_mod, idl)
            else:
                row = image_metrics_torch(pred, gt, l2, self.criterionLPIPS, vgg, id_mod, idl)
            cols = list(row.unbind(0))
        if loss_dict:
            keys = ('loss_l2', 'loss_id', 'loss_lpips', 'loss', 'mae', 'PSNR', 'SSIM', 'ID_SIM')
            return cols[3], dict(zip(keys, cols))
        return cols[3], cols[0], cols[2], cols[1], 0, 0

    def forward(self, *args, **kwargs):
        return self.calc_2d_rec_loss(*args, **kwargs)
