"""Surface extraction, device half: mirrors project/utils/mesh_utils.py of the reference.

    align_volume(volume, near=0.88, far=1.12)        mesh_utils.py:17-44, one HIP kernel (e3dge_align_volume)
    frustum_tables(h, w, d, near, far, device)       the four linspace tables the kernel takes, cached per shape
    marching_cubes_mesh(aligned_sdf)                 the CPU step that follows it (volume_renderer.py:1733-1758): skimage +
                                                     trimesh, third-party and outside the path -- raises ImportError with that
                                                     message when they are not installed
    marching_cubes(aligned_sdf)                      the same step in HIP (e3dge_marching_cubes_*): (verts, faces) on the device
    SurfaceMesh(vertices, faces)                     the part of trimesh.Trimesh the reference's runners use (.vertices, .faces,
                                                     .export(..., file_type='obj'))

The renderer calls align_volume for `return_mesh=True` (volume_renderer.py:1703-1731 of the reference) and returns the aligned
volume as 'aligned_sdf', and marching_cubes' result as 'mesh_verts' / 'mesh_faces'.  'mesh' comes from marching_cubes_mesh when
scikit-image and trimesh are installed, otherwise from the HIP result."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

_TABLES = {}


def frustum_tables(h, w, d, near, far, device):
    """xs (w), ys (h), zs (d) = linspace(-1, 1, n) and coef (d) = linspace(far / near, 1, d): torch.linspace on the host, so
    the values are the reference's own (:20-28)."""
    key = (int(h), int(w), int(d), float(near), float(far), str(device))
    t = _TABLES.get(key)
    if t is None:
        t = tuple(x.to(device) for x in (torch.linspace(-1, 1, w), torch.linspace(-1, 1, h), torch.linspace(-1, 1, d),
                                         torch.linspace(far / near, 1, d)))
        if len(_TABLES) > 16:
            _TABLES.clear()
        _TABLES[key] = t
    return t


def align_volume(volume, near=0.88, far=1.12):
    """(b, h, w, d, c) sampling volume along the camera frustum -> the same shape on the regular grid; voxels outside the
    frustum become 1.  CUDA tensors: e3dge_align_volume; CPU tensors: grid_sample, as the reference does."""
    if volume.dim() != 5:
        raise RuntimeError(f"align_volume expects (b, h, w, d, c), got {tuple(volume.shape)}")
    b, h, w, d, c = volume.shape
    xs, ys, zs, coef = frustum_tables(h, w, d, near, far, volume.device)
    if not volume.is_cuda:
        gx = (xs.view(1, 1, w) * coef.view(d, 1, 1)).expand(d, h, w)
        gy = (ys.view(1, h, 1) * coef.view(d, 1, 1)).expand(d, h, w)
        gz = zs.view(d, 1, 1).expand(d, h, w)
        grid = torch.stack([gx, gy, gz], -1).unsqueeze(0).expand(b, d, h, w, 3).to(volume.dtype)
        out = F.grid_sample(volume.permute(0, 4, 3, 1, 2), grid, padding_mode="border", align_corners=True)
        out = out.permute(0, 3, 4, 2, 1).contiguous()
        outside = ((grid < -1) | (grid > 1)).any(-1)[0].permute(1, 2, 0)                      # (h, w, d)
        return torch.where(outside.view(1, h, w, d, 1), torch.ones((), dtype=out.dtype), out)
    if volume.dtype != torch.float32:
        raise RuntimeError(f"align_volume: float32 expected on the GPU, got {volume.dtype}")
    vol = volume.detach().contiguous()
    out = torch.empty_like(vol)
    with torch.cuda.device(vol.device):
        rc = _lib.load().e3dge_align_volume(_lib.ptr(out), _lib.ptr(vol), _lib.ptr(xs), _lib.ptr(ys), _lib.ptr(zs),
                                            _lib.ptr(coef), b, h, w, d, c, _lib.stream_of(vol))
    _lib.check(rc, "e3dge_align_volume")
    return out


def marching_cubes_mesh(aligned_sdf):
    """The reference's _extract_mesh_with_marching_cubes (volume_renderer.py:1733-1758) on an aligned (1, h, w, d, 1) volume:
    (mesh, verts, faces).  skimage / trimesh are third-party CPU code outside the path."""
    try:
        from skimage.measure import marching_cubes
        import trimesh
    except ImportError as e:
        raise ImportError("marching cubes needs scikit-image and trimesh (CPU, third-party, outside the accelerated path); "
                          "pass 'aligned_sdf' to your own extractor") from e
    _, h, w, d, _ = aligned_sdf.shape
    vol = aligned_sdf[0, ..., 0].permute(1, 0, 2).cpu().numpy()             # (y, x, z) -> (x, y, z)
    verts, faces, _, _ = marching_cubes(vol, 0)
    for axis, n in enumerate((w, h, d)):
        verts[:, axis] = (verts[:, axis] / float(n) - 0.5) * 0.24            # back to the scene scale [-0.12, 0.12]
    verts[:, 2] *= -1
    verts[:, 1] *= -1
    return trimesh.Trimesh(verts, faces), verts, faces


class NoSurfaceError(RuntimeError):
    """skimage's RuntimeError('No surface found at the given iso value.'), as its own type so that callers can tell it from a failing
    launch."""


def marching_cubes(aligned_sdf, scene=True):
    """Marching cubes at level 0 on sample 0, channel 0 of an aligned (b, h, w, d, c) volume, in HIP: (verts (V, 3) float32, faces
    (F, 3) int32), device tensors.  The contract of include/e3dge_hip.h (e3dge_marching_cubes_count): skimage.measure.marching_cubes(
    sdf[0, ..., 0].permute(1, 0, 2), 0) with one vertex per crossing grid edge, then the reference's scene transform
    (volume_renderer.py:1747-1755); scene=False returns skimage's index-space vertices instead.  The volume is read through its strides.

    Errors mirror skimage's: ValueError for a volume smaller than 2x2x2 or a level outside [min, max], NoSurfaceError (a RuntimeError)
    when no edge crosses 0.  The two totals are read back between the count and the emit launches (one 8-byte device-to-host copy,
    which waits for the stream): the call cannot be captured in a HIP graph."""
    if not isinstance(aligned_sdf, torch.Tensor) or aligned_sdf.dim() != 5:
        raise RuntimeError(f"marching_cubes expects an aligned (b, h, w, d, c) volume, got {getattr(aligned_sdf, 'shape', type(aligned_sdf))}")
    _, h, w, d, _ = aligned_sdf.shape
    if min(h, w, d) < 2:
        raise ValueError("Input array must be at least 2x2x2.")
    _lib.require_gpu(aligned_sdf, "marching_cubes: aligned_sdf")
    vol = aligned_sdf.detach()[0, ..., 0]                                    # (h, w, d) view: skimage's (x, y, z) = (w, h, d)
    sy, sx, sz = vol.stride()
    dev = vol.device
    lib = _lib.load()
    nbytes = lib.e3dge_marching_cubes_ws_bytes(w, h, d)
    if nbytes < 0:
        raise RuntimeError(f"marching_cubes: a {h} x {w} x {d} volume is too large for the 32-bit offsets")
    with _lib.on_device(dev):
        stream = _lib.stream_of(vol)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int32, device=dev)
        _lib.check(lib.e3dge_marching_cubes_count(_lib.ptr(totals), _lib.ptr(ws), nbytes, _lib.ptr(vol), w, h, d, sx, sy, sz, stream),
                   "e3dge_marching_cubes_count")
        nv, nf = totals.tolist()
        if nv < 0:
            raise ValueError("Surface level must be within volume data range.")
        if nv == 0:
            raise NoSurfaceError('No surface found at the given iso value.')
        verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
        _lib.check(lib.e3dge_marching_cubes_emit(_lib.ptr(verts), _lib.ptr(faces), nv, nf, _lib.ptr(ws), nbytes, _lib.ptr(vol), w, h, d,
                                                 sx, sy, sz, 1 if scene else 0, stream), "e3dge_marching_cubes_emit")
    return verts, faces


def marching_cubes_tables():
    """The library's case tables: (n_tris (256,), tri_edges (256, MC_MAX_TRIS, 3), -1 past n_tris[c]) as int32 numpy arrays; the corner
    and edge numbering is in include/e3dge_hip.h."""
    n_tris = np.zeros(256, np.int32)
    tri = np.zeros((256, _lib.MC_MAX_TRIS, 3), np.int32)
    _lib.check(_lib.load().e3dge_marching_cubes_tables(n_tris.ctypes.data, tri.ctypes.data), "e3dge_marching_cubes_tables")
    return n_tris, tri


class SurfaceMesh:
    """What the reference's runners use of trimesh.Trimesh (trainer.py:1463-1466): .vertices (V, 3) float32, .faces (F, 3) int32
    (numpy) and .export(file_obj, file_type='obj')."""

    def __init__(self, vertices, faces):
        as_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        self.vertices = np.ascontiguousarray(as_np(vertices), dtype=np.float32)
        self.faces = np.ascontiguousarray(as_np(faces), dtype=np.int32)

    def export(self, file_obj=None, file_type='obj'):
        """Wavefront OBJ: `v x y z` lines (9 significant digits: float32 values read back exactly), then `f i j k` lines (1-based).
        file_obj: a path, a text or binary file object, or None to return the text."""
        if file_type != 'obj':
            raise ValueError(f"SurfaceMesh exports 'obj' only, not {file_type!r}")
        lines = ["v %.9g %.9g %.9g" % tuple(v) for v in self.vertices.tolist()]
        lines += ["f %d %d %d" % tuple(f) for f in (self.faces.astype(np.int64) + 1).tolist()]
        text = "\n".join(lines) + "\n"
        if file_obj is None:
            return text
        if isinstance(file_obj, (str, bytes)) or hasattr(file_obj, "__fspath__"):
            with open(file_obj, "w") as f:
                f.write(text)
        else:
            try:
                file_obj.write(text)
            except TypeError:                                               # a binary file object
                file_obj.write(text.encode())
        return text


def mesh_from_hip(verts, faces):
    """'mesh' for the renderer when skimage is missing: trimesh.Trimesh(verts, faces) if trimesh imports (the reference's call,
    volume_renderer.py:1757), else a SurfaceMesh."""
    try:
        import trimesh
    except ImportError:
        return SurfaceMesh(verts, faces)
    return trimesh.Trimesh(verts.cpu().numpy(), faces.cpu().numpy())


@functools.lru_cache(maxsize=None)
def third_party_available():
    """scikit-image and trimesh both import (checked once per process)."""
    try:
        import skimage.measure  # noqa: F401
        import trimesh  # noqa: F401
    except ImportError:
        return False
    return True
