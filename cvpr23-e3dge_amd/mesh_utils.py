"""Surface extraction, device half: mirrors project/utils/mesh_utils.py of the reference.

    align_volume(volume, near=0.88, far=1.12)        mesh_utils.py:17-44, one HIP kernel (e3dge_align_volume)
    frustum_tables(h, w, d, near, far, device)       the four linspace tables the kernel takes, cached per shape
    marching_cubes_mesh(aligned_sdf)                 the CPU step that follows it (volume_renderer.py:1733-1758): skimage +
                                                     trimesh, third-party and outside the path -- raises ImportError with that
                                                     message when they are not installed
    marching_cubes(aligned_sdf)                      the same step in HIP (e3dge_marching_cubes_*): (verts, faces) on the device
    SurfaceMesh(vertices, faces)                     the part of trimesh.Trimesh the reference's runners use (.vertices, .faces,
                                                     .export(..., file_type='obj'))

Surface renderings (mesh_utils.py:107-173 and trainer.py:1482-1534, 2254-2346 of the reference; csrc/mesh_render.hip):
    depth_mesh(xyz) / xyz2mesh(xyz)                  the renderer's xyz map as a triangle mesh: device tensors / the reference's return
    vertex_normals(verts, faces)                     angle-weighted vertex normals (what trimesh's .vertex_normals feeds pytorch3d)
    MeshCamera(azim, elev, fov, ...)                 create_cameras (camera_utils.py:158-179) on the host: twelve floats
    create_mesh_renderer / create_depth_mesh_renderer   the pytorch3d Phong renderer as one HIP rasteriser (e3dge_mesh_render)
    render_depth_mesh(xyz, viewpoint) / render_surface_mesh(verts, faces, viewpoint)   the runner's two geometry images

View-consistent decoder noise (NoiseInjection.project_noise, project/models/stylesdf_model.py:365-466 of the reference):
    pose_to_viewpoint(c2w)                           (azim, elev) of a camera pose: pytorch3d's matrix_to_euler_angles(.., "ZYX") on the host
    subdivide(verts, faces, levels)                  midpoint subdivision (trimesh.remesh.subdivide) in HIP (e3dge_mesh_subdivide)
    load_mesh(mesh)                                  an OBJ path, a SurfaceMesh or a (verts, faces) pair -> LoadedMesh, levels cached
    project_vertex_noise(verts, faces, vert_noise, camera, image_size, prev)   the 17-fragment soft blend of per-vertex noise
                                                     (e3dge_noise_project): (maps, valid)

The renderer calls align_volume for `return_mesh=True` (volume_renderer.py:1703-1731 of the reference) and returns the aligned
volume as 'aligned_sdf', and marching_cubes' result as 'mesh_verts' / 'mesh_faces'.  'mesh' comes from marching_cubes_mesh when
scikit-image and trimesh are installed, otherwise from the HIP result."""
import functools
import os

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
    _lib.launch("e3dge_align_volume", out, vol, xs, ys, zs, coef, b, h, w, d, c)
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
    nbytes = _lib.load().e3dge_marching_cubes_ws_bytes(w, h, d)
    if nbytes < 0:
        raise RuntimeError(f"marching_cubes: a {h} x {w} x {d} volume is too large for the 32-bit offsets")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.launch("e3dge_marching_cubes_count", totals, ws, nbytes, vol, w, h, d, sx, sy, sz)
    nv, nf = totals.tolist()
    if nv < 0:
        raise ValueError("Surface level must be within volume data range.")
    if nv == 0:
        raise NoSurfaceError('No surface found at the given iso value.')
    verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    _lib.launch("e3dge_marching_cubes_emit", verts, faces, nv, nf, ws, nbytes, vol, w, h, d, sx, sy, sz, 1 if scene else 0)
    return verts, faces


def marching_cubes_tables():
    """The library's case tables: (n_tris (256,), tri_edges (256, MC_MAX_TRIS, 3), -1 past n_tris[c]) as int32 numpy arrays; the corner
    and edge numbering is in include/e3dge_hip.h."""
    n_tris = np.zeros(256, np.int32)
    tri = np.zeros((256, _lib.MC_MAX_TRIS, 3), np.int32)
    lib = _lib.load()
    if lib.e3dge_marching_cubes_tables(n_tris.ctypes.data, tri.ctypes.data) != 0:      # (no stream, nothing queued: a plain call)
        raise RuntimeError("e3dge_marching_cubes_tables: " + lib.e3dge_last_error().decode(errors="replace"))
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


# ---- surface renderings -----------------------------------------------------------------------------------------------------------------
def depth_mesh_faces(h, w):
    """The face list of depth_mesh on the host, in the order include/e3dge_hip.h documents: cell (r, c) in row-major order gives
    (r w + c, (r+1) w + c, r w + c + 1) then ((r+1) w + c, (r+1) w + c + 1, r w + c + 1).  (2 (h-1)(w-1), 3) int32."""
    r, c = np.meshgrid(np.arange(h - 1), np.arange(w - 1), indexing="ij")
    a = (r * w + c).reshape(-1)
    b = a + w
    return np.stack([np.stack([a, b, a + 1], 1), np.stack([b, b + 1, a + 1], 1)], 1).reshape(-1, 3).astype(np.int32)


def depth_mesh(xyz):
    """xyz (1, 3, h, w) float32 on the GPU (the renderer's 'xyz') -> verts (h w, 3) float32, faces (2 (h-1)(w-1), 3) int32: xyz2mesh
    (mesh_utils.py:107-126) with one fixed diagonal per cell and the reference's winding.  One launch, no host round trip."""
    _lib.require_gpu(xyz, "depth_mesh: xyz")
    if xyz.dim() != 4 or xyz.shape[0] != 1 or xyz.shape[1] != 3:
        raise RuntimeError(f"depth_mesh expects (1, 3, h, w), got {tuple(xyz.shape)}")
    _, _, h, w = xyz.shape
    src = xyz.detach().contiguous()
    verts = torch.empty(h * w, 3, dtype=torch.float32, device=src.device)
    faces = torch.empty(2 * (h - 1) * (w - 1), 3, dtype=torch.int32, device=src.device)
    _lib.launch("e3dge_depth_mesh", verts, faces, src, h, w)
    return verts, faces


def xyz2mesh(xyz):
    """The reference's xyz2mesh: a trimesh.Trimesh when trimesh imports, otherwise a SurfaceMesh (as mesh_from_hip decides).  Accepts a
    numpy array or a CPU tensor like the reference; the mesh is built on the GPU."""
    if not isinstance(xyz, torch.Tensor):
        xyz = torch.from_numpy(np.asarray(xyz))
    if not xyz.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("xyz2mesh builds the mesh on the GPU (HIP); this build has no CPU path")
        xyz = xyz.cuda()
    return mesh_from_hip(*depth_mesh(xyz.float()))


def _mesh_args(verts, faces, what):
    _lib.require_gpu(verts, f"{what}: verts")
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise RuntimeError(f"{what}: verts must be (V, 3), got {tuple(verts.shape)}")
    if not isinstance(faces, torch.Tensor) or faces.device != verts.device or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError(f"{what}: faces must be an (F, 3) tensor on the device of verts")
    return verts.detach().contiguous(), faces.detach().to(torch.int32).contiguous()


def vertex_normals(verts, faces):
    """(V, 3) float32 unit normals: the sum over a vertex's faces of the unit face normal weighted by the face's corner angle at the
    vertex, normalised; (0, 0, 0) for a vertex without faces.  Bit-reproducible (include/e3dge_hip.h, e3dge_vertex_normals)."""
    verts, faces = _mesh_args(verts, faces, "vertex_normals")
    nv, nf = verts.shape[0], faces.shape[0]
    nbytes = _lib.load().e3dge_vertex_normals_ws_bytes(nv)
    out = torch.empty_like(verts)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=verts.device)
    _lib.launch("e3dge_vertex_normals", out, verts, faces, nv, nf, ws, nbytes)
    return out


class MeshCamera:
    """create_cameras (camera_utils.py:158-179) on the host: a camera at distance `dist` from the origin, looking at it, `azim` / `elev`
    in degrees, `fov` the FULL field of view in degrees.  View coordinates: +x left, +y up, +z into the scene; NDC = view.xy / (view.z
    tan(fov / 2)); the centre of pixel (row i, column j) of an S x S image is (1 - (2 j + 1) / S, 1 - (2 i + 1) / S).  The same rays as
    generate_camera_params + get_rays at (azim, elev) with fov = 2 fov_ang.  float64 on the host; `floats()` is what the kernel takes."""

    def __init__(self, azim, elev, fov, dist=1.0, znear=0.01, zfar=100.0):
        a, e = np.deg2rad(float(azim)), np.deg2rad(float(elev))
        self.fov, self.dist, self.znear, self.zfar = float(fov), float(dist), float(znear), float(zfar)
        self.position = self.dist * np.array([np.cos(e) * np.sin(a), np.sin(e), np.cos(e) * np.cos(a)])
        unit = lambda v: v / np.linalg.norm(v)
        self.z_ax = unit(-self.position)
        self.x_ax = unit(np.cross(np.array([0.0, 1.0, 0.0]), self.z_ax))
        self.y_ax = np.cross(self.z_ax, self.x_ax)
        self.tan_half_fov = float(np.tan(np.deg2rad(self.fov) / 2))

    def view(self, points):
        """(..., 3) world points -> view coordinates (float64)."""
        d = np.asarray(points, np.float64) - self.position
        return np.stack([d @ self.x_ax, d @ self.y_ax, d @ self.z_ax], -1)

    def project(self, points):
        """(..., 3) world points -> (x_n, y_n, view z)."""
        v = self.view(points)
        return np.stack([v[..., 0] / (v[..., 2] * self.tan_half_fov), v[..., 1] / (v[..., 2] * self.tan_half_fov), v[..., 2]], -1)

    def pixels(self, points, image_size):
        """(..., 3) world points -> fractional (row, column): a pixel's centre maps to its integer index."""
        p = self.project(points)
        return np.stack([((1 - p[..., 1]) * image_size - 1) / 2, ((1 - p[..., 0]) * image_size - 1) / 2], -1)

    def floats(self):
        """C, x_ax, y_ax, z_ax: the twelve float32 of E3dgeMeshRenderArgs.camera."""
        return np.concatenate([self.position, self.x_ax, self.y_ax, self.z_ax]).astype(np.float32)


def _rgb(value, name):
    v = np.asarray(value, np.float32).reshape(-1)
    if v.size != 3:
        raise ValueError(f"{name} must be ((r, g, b),), got {value!r}")
    return v


class MeshRenderer:
    """What create_mesh_renderer returns: renderer(verts, faces, normals=None, colors=None) -> image (1, S, S, 4).  `rasterize` also
    returns zbuf (S, S, K) and pix_to_face (S, S, K)."""
    SIGMA = GAMMA = 1e-4                # pytorch3d's BlendParams defaults, as is the white background
    BACKGROUND = (1.0, 1.0, 1.0)

    def __init__(self, camera, image_size=256, blur_radius=1e-6, light_location=((-0.5, 1., 5.),), faces_per_pixel=5,
                 ambient_color=((0.5, 0.5, 0.5),), diffuse_color=((0.3, 0.3, 0.3),), specular_color=((0.2, 0.2, 0.2),)):
        if not isinstance(camera, MeshCamera):
            raise TypeError("create_mesh_renderer takes a MeshCamera (mesh_utils.MeshCamera(azim, elev, fov))")
        if not 1 <= int(faces_per_pixel) <= _lib.MESH_MAX_FACES_PER_PIXEL:
            raise ValueError(f"faces_per_pixel = {faces_per_pixel}: the HIP rasteriser keeps 1..{_lib.MESH_MAX_FACES_PER_PIXEL} fragments "
                             "per pixel in registers")
        if int(image_size) < 1:
            raise ValueError(f"image_size = {image_size}")
        self.camera, self.image_size, self.blur_radius = camera, int(image_size), float(blur_radius)
        self.faces_per_pixel = int(faces_per_pixel)
        self.light_location = _rgb(light_location, "light_location")
        self.ambient_color, self.diffuse_color = _rgb(ambient_color, "ambient_color"), _rgb(diffuse_color, "diffuse_color")
        self.specular_color = _rgb(specular_color, "specular_color")
        self.bin_factor = 4

    def _args(self):
        a = _lib.MeshRenderArgs()
        a.camera[:] = self.camera.floats().tolist()
        a.tan_half_fov, a.znear, a.zfar = self.camera.tan_half_fov, self.camera.znear, self.camera.zfar
        for name in ("light_location", "ambient_color", "diffuse_color", "specular_color"):
            getattr(a, name)[:] = getattr(self, name).tolist()
        a.background_color[:] = self.BACKGROUND
        a.blur_radius, a.sigma, a.gamma = self.blur_radius, self.SIGMA, self.GAMMA
        a.image_size, a.faces_per_pixel = self.image_size, self.faces_per_pixel
        return a

    def rasterize(self, verts, faces, normals=None, colors=None, bin_capacity=None):
        """(image (S, S, 4), zbuf (S, S, K), pix_to_face (S, S, K)).  The status word is read back after the launch (one 8-byte copy):
        when the per-tile face lists did not fit `bin_capacity` entries (default: 4 per face + 64 per tile) the call is repeated once
        with what they need; a `bin_capacity` given by the caller is not grown -- the call raises instead."""
        verts, faces = _mesh_args(verts, faces, "mesh renderer")
        if normals is None:
            normals = vertex_normals(verts, faces)
        for t, name in ((normals, "normals"), (colors, "colors")):
            if t is not None:
                _lib.require_gpu(t, f"mesh renderer: {name}")
                if t.shape != verts.shape or t.device != verts.device:
                    raise RuntimeError(f"mesh renderer: {name} must be (V, 3) on the device of verts, got {tuple(t.shape)}")
        normals = normals.detach().contiguous()
        colors = None if colors is None else colors.detach().contiguous()
        dev, S, K = verts.device, self.image_size, self.faces_per_pixel
        nv, nf = verts.shape[0], faces.shape[0]
        tiles = ((S + 15) // 16) ** 2
        fixed = bin_capacity is not None
        cap = int(bin_capacity) if fixed else self.bin_factor * nf + 64 * tiles
        image = torch.empty(S, S, 4, dtype=torch.float32, device=dev)
        zbuf = torch.empty(S, S, K, dtype=torch.float32, device=dev)
        pix = torch.empty(S, S, K, dtype=torch.int32, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        a = self._args()
        a.verts, a.faces, a.normals, a.colors = verts, faces, normals, colors
        a.n_verts, a.n_faces = nv, nf
        a.image, a.zbuf, a.pix_to_face, a.status = image, zbuf, pix, status
        for attempt in range(2):
            cap = min(cap, nf * tiles)
            nbytes = _lib.query("e3dge_mesh_render_ws_bytes", nv, nf, S, cap)
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
            a.ws, a.ws_bytes, a.bin_capacity = ws, nbytes, cap
            _lib.launch("e3dge_mesh_render", a)
            need, _ = status.tolist()
            if need <= cap:
                return image, zbuf, pix
            if fixed:
                break
            cap = need
        raise RuntimeError(f"mesh renderer: the tile lists need {need} entries, bin_capacity is {cap}")

    def __call__(self, verts, faces, normals=None, colors=None):
        return self.rasterize(verts, faces, normals, colors)[0].unsqueeze(0)


class DepthMeshRenderer(MeshRenderer):
    """create_depth_mesh_renderer's return: renderer(verts, faces, ...) -> (image (1, S, S, 4), zbuf (1, S, S, K))."""

    def __call__(self, verts, faces, normals=None, colors=None):
        image, zbuf, _ = self.rasterize(verts, faces, normals, colors)
        return image.unsqueeze(0), zbuf.unsqueeze(0)


def create_mesh_renderer(camera, image_size=256, blur_radius=1e-6, light_location=((-0.5, 1., 5.),), faces_per_pixel=5, **light_kwargs):
    """The reference's create_mesh_renderer (mesh_utils.py:145-173): pytorch3d's MeshRasterizer + SoftPhongShader with PointLights
    (ambient_color 0.5, diffuse_color 0.3, specular_color 0.2 unless given, each ((r, g, b),)), as one HIP rasteriser.  `camera`: a
    MeshCamera."""
    return MeshRenderer(camera, image_size, blur_radius, light_location, faces_per_pixel, **light_kwargs)


def create_depth_mesh_renderer(camera, image_size=256, blur_radius=1e-6, light_location=((-0.5, 1., 5.),), faces_per_pixel=5,
                               **light_kwargs):
    """The reference's create_depth_mesh_renderer: the same renderer returning (image, zbuf).  The reference asks for 17 faces per pixel
    there; it only serves noise projection, which has its own entry here (project_vertex_noise / e3dge_noise_project, 17 fragments per
    pixel and no zbuf output): more than 8 is refused by this one."""
    return DepthMeshRenderer(camera, image_size, blur_radius, light_location, faces_per_pixel, **light_kwargs)


def _viewpoint_camera(viewpoint, fov_ang):
    v = viewpoint.detach().cpu().numpy() if isinstance(viewpoint, torch.Tensor) else np.asarray(viewpoint)
    v = v.reshape(-1).astype(np.float64)
    if v.size != 2:
        raise ValueError(f"viewpoint must be one (azim, elev) pair in radians, got shape {v.shape}")
    return MeshCamera(azim=np.rad2deg(v[0]), elev=np.rad2deg(v[1]), fov=2 * fov_ang, dist=1)


_RUNNER_LIGHTS = dict(specular_color=((0.2, 0.2, 0.2),), ambient_color=((0.1, 0.1, 0.1),), diffuse_color=((0.65, .65, .65),))


def render_depth_mesh(xyz, viewpoint, fov_ang=6.0, image_size=512):
    """The geometry image of AERunner.render_depth_mesh (trainer.py:2295-2331): the depth mesh of `xyz` (1, 3, h, w), shaded from
    `viewpoint` = (azim, elev) in radians as generate_camera_params returns it -> (S, S, 3) float32 in 0..255 on the device.  The
    runner's background mask (:2283-2289, 2332-2337) is the caller's."""
    verts, faces = depth_mesh(xyz)
    r = create_mesh_renderer(_viewpoint_camera(viewpoint, fov_ang), image_size=image_size, light_location=((0.0, 0.0, 5.0),), **_RUNNER_LIGHTS)
    return 255 * r(verts, faces)[0, ..., :3]


def render_surface_mesh(verts, faces, viewpoint, fov_ang=6.0, image_size=512, colors=None):
    """AERunner.render_trimesh (trainer.py:1482-1534) for a marching-cubes mesh on the device -> (S, S, 3) float32 in 0..255."""
    r = create_mesh_renderer(_viewpoint_camera(viewpoint, fov_ang), image_size=image_size, light_location=((0.0, 3.0, 5.0),), **_RUNNER_LIGHTS)
    return 255 * r(verts, faces, colors=colors)[0, ..., :3]


# ---- view-consistent decoder noise -------------------------------------------------------------------------------------------------------
def pose_to_viewpoint(c2w):
    """(azim, elev) in radians of a camera pose (3, 4) or (b, 3, 4) -- sample 0 -- as NoiseInjection.project_noise reads it
    (stylesdf_model.py:427-429 of the reference): angles = matrix_to_euler_angles(R, "ZYX") with R = Rz(a0) Ry(a1) Rx(a2), azim = a1 =
    asin(-R[2, 0]), elev = -a2 = -atan2(R[2, 1], R[2, 2]).  float64 on the host; for generate_camera_params' poses it returns the
    viewpoint they were built from."""
    R = c2w.detach().cpu().double().numpy() if isinstance(c2w, torch.Tensor) else np.asarray(c2w, np.float64)
    if R.ndim == 3:
        R = R[0]
    if R.ndim != 2 or R.shape[0] != 3 or R.shape[1] < 3:
        raise ValueError(f"pose_to_viewpoint expects a (3, 4) or (b, 3, 4) camera-to-world matrix, got {np.shape(c2w)}")
    return float(np.arcsin(np.clip(-R[2, 0], -1.0, 1.0))), float(-np.arctan2(R[2, 1], R[2, 2]))


def _subdivide_once(verts, faces):
    nv, nf = verts.shape[0], faces.shape[0]
    f = faces.to(torch.int64)
    a, b = f, f.roll(-1, 1)                                                       # sides (a, b), (b, c), (c, a)
    keys = torch.minimum(a, b) * nv + torch.maximum(a, b)                        # lo V + hi
    edge_keys, rank = torch.unique(keys.reshape(-1), sorted=True, return_inverse=True)      # ranking the 3 F keys: torch's sort
    ne = edge_keys.shape[0]
    if nv + ne >= 2 ** 31 or 4 * nf >= 2 ** 31:
        raise RuntimeError(f"subdivide: {nv + ne} vertices, {4 * nf} faces exceed the 32-bit indices")
    rank = rank.to(torch.int32).contiguous()
    out_v = torch.empty(nv + ne, 3, dtype=torch.float32, device=verts.device)
    out_f = torch.empty(4 * nf, 3, dtype=torch.int32, device=verts.device)
    _lib.launch("e3dge_mesh_subdivide", out_v, out_f, verts, faces, edge_keys, rank, nv, nf, ne)
    return out_v, out_f


def subdivide(verts, faces, levels=1):
    """`levels` rounds of midpoint subdivision (trimesh.remesh.subdivide) on the device: every edge gets a vertex at its midpoint, every
    face becomes four, the winding is kept.  The order of the new vertices and faces is the one include/e3dge_hip.h documents
    (e3dge_mesh_subdivide): new vertex V + rank of the edge key lo V + hi.  Face indices must lie in [0, V)."""
    verts, faces = _mesh_args(verts, faces, "subdivide")
    if int(levels) < 0:
        raise ValueError(f"subdivide: levels = {levels}")
    for _ in range(int(levels)):
        verts, faces = _subdivide_once(verts, faces)
    return verts, faces


def subdivision_level(image_size):
    """The number of subdivisions NoiseInjection.load_mc_mesh applies for a noise map of this size (stylesdf_model.py:394-421 of the
    reference): 64 and 128 none, 256 one, everything else three.  The reference's return after two subdivisions tests `im_res == 256` a
    second time and is never reached; no size gets level 2 here either."""
    return 0 if image_size in (64, 128) else 1 if image_size == 256 else 3


def read_obj(path):
    """(vertices (V, 3) float32, faces (F, 3) int32) of a Wavefront OBJ of `v x y z` / `f i j k` lines, as SurfaceMesh.export writes it
    (`i/t/n` corners are read by their vertex index; other lines are skipped)."""
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                v.append([float(x) for x in p[1:4]])
            elif p[0] == "f":
                if len(p) != 4:
                    raise ValueError(f"{path}: only triangles are read, got {line.strip()!r}")
                f.append([int(x.split("/")[0]) - 1 for x in p[1:4]])
    return np.asarray(v, np.float64).reshape(-1, 3).astype(np.float32), np.asarray(f, np.int64).reshape(-1, 3).astype(np.int32)


class LoadedMesh:
    """A mesh on the device with its subdivision levels, each computed on first use and kept: level(n) -> (verts, faces)."""

    def __init__(self, verts, faces):
        self.levels = {0: _mesh_args(verts, faces, "load_mesh")}

    def level(self, n):
        if n not in self.levels:
            base = max(k for k in self.levels if k < n)
            v, f = self.levels[base]
            for k in range(base + 1, n + 1):
                v, f = subdivide(v, f, 1)
                self.levels[k] = (v, f)
        return self.levels[n]

    def for_image(self, image_size):
        return self.level(subdivision_level(image_size))


_MESHES = {}                        # key -> (what the key was made from, LoadedMesh): the last few meshes


def load_mesh(mesh, device="cuda"):
    """What NoiseInjection's `mesh_path` may be -> LoadedMesh: a path to a Wavefront OBJ as SurfaceMesh.export writes it, a SurfaceMesh
    (or anything with .vertices / .faces), or a (verts, faces) pair of device tensors.  The result, with the subdivision levels it has
    computed, is cached per mesh: per (path, modification time), per object, per pair of tensors (identity, pointer and version)."""
    if isinstance(mesh, (str, bytes)) or hasattr(mesh, "__fspath__"):
        path = os.path.abspath(os.fsdecode(mesh))
        st = os.stat(path)
        key, held = ("path", path, st.st_mtime_ns, st.st_size, str(device)), None
    elif isinstance(mesh, (tuple, list)) and len(mesh) == 2 and all(isinstance(t, torch.Tensor) for t in mesh):
        key, held = ("pair",) + tuple((id(t), t.data_ptr(), t._version) for t in mesh), tuple(mesh)
    elif hasattr(mesh, "vertices") and hasattr(mesh, "faces"):
        key, held = ("object", id(mesh), str(device)), mesh
    else:
        raise TypeError("mesh_path must be an OBJ path, a mesh with .vertices / .faces or a (verts, faces) pair of device tensors, got "
                        f"{type(mesh).__name__}")
    hit = _MESHES.get(key)
    if hit is not None:
        return hit[1]
    if key[0] == "pair":
        loaded = LoadedMesh(mesh[0], mesh[1])
    else:
        v, f = read_obj(key[1]) if key[0] == "path" else (np.asarray(mesh.vertices, np.float32), np.asarray(mesh.faces).astype(np.int32))
        loaded = LoadedMesh(torch.from_numpy(np.ascontiguousarray(v)).to(device), torch.from_numpy(np.ascontiguousarray(f)).to(device))
    while len(_MESHES) >= 4:                                                     # a video uses one mesh per identity
        _MESHES.pop(next(iter(_MESHES)))
    _MESHES[key] = (held, loaded)                                                # `held` keeps the ids of the key alive
    return loaded


def project_vertex_noise(verts, faces, vert_noise, camera, image_size, prev=None, bin_capacity=None):
    """vert_noise (C, V) or (V,) float32 on the device, 1 <= C <= 4: scalar fields over the vertices -> (maps (C, S, S) float32, valid
    (S, S) bool).  maps = the soft blend of the 17 nearest fragments' interpolated values as the reference's create_depth_mesh_renderer
    gives it (blur_radius 1e-6, ambient 1, BlendParams defaults) where valid, `prev` (C, S, S) -- zeros when None -- elsewhere.  One
    rasterisation for all C maps (e3dge_noise_project).  The bin protocol is MeshRenderer.rasterize's: one retry with the capacity the
    status word asks for."""
    verts, faces = _mesh_args(verts, faces, "project_vertex_noise")
    if not isinstance(camera, MeshCamera):
        raise TypeError("project_vertex_noise takes a MeshCamera (mesh_utils.MeshCamera(azim, elev, fov))")
    S = int(image_size)
    if S < 1:
        raise ValueError(f"image_size = {image_size}")
    _lib.require_gpu(vert_noise, "project_vertex_noise: vert_noise")
    nv, nf, dev = verts.shape[0], faces.shape[0], verts.device
    vn = vert_noise.detach().reshape(-1, nv).contiguous() if vert_noise.numel() and vert_noise.shape[-1] == nv else None
    if vn is None or vert_noise.device != dev or vert_noise.dim() > 2 or not 1 <= vn.shape[0] <= _lib.NOISE_PROJECT_MAX_MAPS:
        raise RuntimeError(f"project_vertex_noise: vert_noise must be (C, {nv}) on the device of verts with 1 <= C <= "
                           f"{_lib.NOISE_PROJECT_MAX_MAPS}, got {tuple(vert_noise.shape)}")
    C = vn.shape[0]
    if prev is None:
        prev = torch.zeros(C, S, S, dtype=torch.float32, device=dev)
    else:
        _lib.require_gpu(prev, "project_vertex_noise: prev")
        if prev.numel() != C * S * S or prev.device != dev:
            raise RuntimeError(f"project_vertex_noise: prev must be ({C}, {S}, {S}) on the device of verts, got {tuple(prev.shape)}")
        prev = prev.detach().contiguous()
    tiles = ((S + 15) // 16) ** 2
    fixed = bin_capacity is not None
    cap = int(bin_capacity) if fixed else 4 * nf + 64 * tiles
    out = torch.empty(C, S, S, dtype=torch.float32, device=dev)
    valid = torch.empty(S, S, dtype=torch.uint8, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    a = _lib.NoiseProjectArgs()
    a.camera[:] = camera.floats().tolist()
    a.tan_half_fov, a.znear, a.zfar = camera.tan_half_fov, camera.znear, camera.zfar
    a.blur_radius, a.sigma, a.gamma = 1e-6, MeshRenderer.SIGMA, MeshRenderer.GAMMA
    a.image_size, a.n_maps, a.n_verts, a.n_faces = S, C, nv, nf
    a.verts, a.faces, a.vert_noise, a.prev = verts, faces, vn, prev
    a.out, a.valid, a.status = out, valid, status
    for attempt in range(2):
        cap = min(cap, nf * tiles, 2 ** 31 - 2)
        nbytes = _lib.query("e3dge_noise_project_ws_bytes", nv, nf, S, cap)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        a.ws, a.ws_bytes, a.bin_capacity = ws, nbytes, cap
        _lib.launch("e3dge_noise_project", a)
        need, _ = status.tolist()
        if need <= cap:
            return out, valid.bool()
        if fixed:
            break
        cap = need
    raise RuntimeError(f"project_vertex_noise: the tile lists need {need} entries, bin_capacity is {cap}")


def noise_camera(transform):
    """The camera NoiseInjection.project_noise draws from (stylesdf_model.py:427-434 of the reference): create_cameras at the pose's
    (azim, elev), fov 12 degrees, distance 1."""
    azim, elev = pose_to_viewpoint(transform)
    return MeshCamera(azim=np.rad2deg(azim), elev=np.rad2deg(elev), fov=12.0, dist=1)
