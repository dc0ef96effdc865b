// Surface extraction, the step after align_volume: marching cubes at level 0 on the aligned SDF volume, and the reference's scene
// transform of the vertices.
//
// Reference: VolumeFeatureRenderer._extract_mesh_with_marching_cubes (project/utils/volume_renderer.py:1733-1758; the same code as
// project/utils/mesh_utils.py:48-70): skimage.measure.marching_cubes(sdf[0, ..., 0].permute(1, 0, 2), 0), then per axis
// (v / n - 0.5) * 0.24 with n = (w, h, d) and y, z negated.  The contract, the numbering and the output order are in
// include/e3dge_hip.h next to e3dge_marching_cubes_count; DESIGN.md 4.12b has the derivation and the measured times.
//
// Four launches, no atomics deciding where anything goes:
//   count   per point: crossing edges it owns (+x, +y, +z) and triangles of the cell it is the origin of; per block of 1024 points
//           the packed sum (vertices low 32 bits, faces high 32 bits) and two sign flags for skimage's range check
//   scan    one block: exclusive scan of the block sums, totals -> the caller's 2-int buffer
//   verts   per block: the per-point counts again, block scan + block offset -> vertex offset of every point (kept in the workspace
//           with the point's crossing mask), vertices written
//   faces   per block: the per-cell triangle counts again, block scan + block offset -> face offset; each triangle corner is the
//           vertex offset of the edge's owner point plus the edge's rank among that point's crossing edges
// Bound: HBM and launch latency.  At 128^3 the volume (8.4 MB) is read three times (the second and third mostly from L2 / MALL), the
// per-point words (8.4 MB) written once and read once, the mesh (< 1 MB) written once.
#include "common.h"

namespace e3dge {

// ---- case tables, generated at compile time ---------------------------------------------------------------------------------------
// Corner k of a cell sits at (dx, dy, dz) = (k & 1, (k >> 1) & 1, (k >> 2) & 1); bit k of the case index is set iff its value is > 0.
// Edge e = 4 * axis + j runs from its lower corner along `axis` (0 = x, 1 = y, 2 = z); j holds the offsets on the two other axes in
// increasing axis order (j & 1 the lower one).  The lower corner owns the edge's vertex.
//
// For each case, on each of the six faces (corners listed counter-clockwise seen from outside the cube), every maximal run of
// positive corners in that cyclic order gives one segment, from the edge where the run is entered to the edge where it is left.  On
// an ambiguous face (+ - + -) the runs are single corners: the positive corners are separated.  The rule sees only the face's own
// signs, so the two cells that share a face draw the same segments, traversed in opposite directions (their cyclic orders are
// reversed): the surface is closed and consistently oriented.  Each crossing edge is entered on one of its two faces and left on the
// other, so the segments chain into loops; each loop, started at its lowest edge, is triangulated by ear clipping (below).  Triangles
// wind against the loop: the right-hand normal then points towards the positive side, as skimage's default
// gradient_direction='descent'.
constexpr int kMcMaxTris = E3DGE_MC_MAX_TRIS;

struct McTables {
    unsigned char n_tris[256];
    signed char tri[256][kMcMaxTris][3];
};

constexpr int mc_edge_of(int a, int b) {
    const int lo = a < b ? a : b;
    const int axis = (a ^ b) == 1 ? 0 : (a ^ b) == 2 ? 1 : 2;
    const int dx = lo & 1, dy = (lo >> 1) & 1, dz = (lo >> 2) & 1;
    const int j = axis == 0 ? dy + 2 * dz : axis == 1 ? dx + 2 * dz : dx + 2 * dy;
    return 4 * axis + j;
}

// Do grid edges a and b of a cell lie on a common face?  Edge 4 * axis + j lies on the two faces fixed by its offsets on the other axes.
constexpr bool mc_share_face(int a, int b) {
    int fa[2] = {0, 0}, fb[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
        const int e = k ? b : a, axis = e >> 2, j = e & 3;
        const int lo = axis == 0 ? 1 : 0, hi = axis == 2 ? 1 : 2;        // the two other axes, lower first
        int* f = k ? fb : fa;
        f[0] = 2 * lo + (j & 1);
        f[1] = 2 * hi + (j >> 1);
    }
    return fa[0] == fb[0] || fa[0] == fb[1] || fa[1] == fb[0] || fa[1] == fb[1];
}

constexpr McTables make_mc_tables() {
    McTables t{};
    const int faces[6][4] = {{0, 4, 6, 2}, {1, 3, 7, 5},     // x = 0, x = 1
                             {0, 1, 5, 4}, {2, 6, 7, 3},     // y = 0, y = 1
                             {0, 2, 3, 1}, {4, 5, 7, 6}};    // z = 0, z = 1
    for (int c = 0; c < 256; ++c) {
        int next[12] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
        for (int f = 0; f < 6; ++f) {
            int pos[4] = {0, 0, 0, 0};
            for (int i = 0; i < 4; ++i) pos[i] = (c >> faces[f][i]) & 1;
            for (int i = 0; i < 4; ++i) {
                if (pos[i] || !pos[(i + 1) & 3]) continue;                 // not the entry of a positive run
                int j = (i + 1) & 3;
                while (pos[(j + 1) & 3]) j = (j + 1) & 3;                  // last positive corner of the run
                next[mc_edge_of(faces[f][i], faces[f][(i + 1) & 3])] = mc_edge_of(faces[f][j], faces[f][(j + 1) & 3]);
            }
        }
        bool seen[12] = {false, false, false, false, false, false, false, false, false, false, false, false};
        int n = 0;
        for (int e0 = 0; e0 < 12; ++e0) {
            if (next[e0] < 0 || seen[e0]) continue;
            int loop[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            int len = 0;
            for (int e = e0; !seen[e]; e = next[e]) {
                seen[e] = true;
                loop[len++] = e;
            }
            // ear clipping from the loop's start: the first ear whose new diagonal does not lie on a cube face (on a convex loop with
            // no ambiguous face this is the fan from loop[0]).  A chord across an ambiguous face could also be drawn by the cell on
            // the other side, and an edge of the mesh would then border four triangles.
            while (len >= 3) {
                int i = 0;
                if (len > 3) {
                    while (i < len && mc_share_face(loop[(i + len - 1) % len], loop[(i + 1) % len])) ++i;
                    if (i == len) i = 0;
                }
                t.tri[c][n][0] = (signed char)loop[(i + len - 1) % len];
                t.tri[c][n][1] = (signed char)loop[(i + 1) % len];
                t.tri[c][n][2] = (signed char)loop[i];
                ++n;
                for (int k = i; k + 1 < len; ++k) loop[k] = loop[k + 1];
                --len;
            }
        }
        t.n_tris[c] = (unsigned char)n;
    }
    return t;
}

constexpr McTables kMcHostTables = make_mc_tables();
__constant__ McTables kMcTables = make_mc_tables();

constexpr int mc_max_tris() {
    int m = 0;
    for (int c = 0; c < 256; ++c) m = kMcHostTables.n_tris[c] > m ? kMcHostTables.n_tris[c] : m;
    return m;
}
static_assert(mc_max_tris() <= kMcMaxTris, "marching cubes: a case has more triangles than the table holds");

// ---- kernels ------------------------------------------------------------------------------------------------------------------------
constexpr int kMcThreads = 256, kMcItems = 4, kMcTile = kMcThreads * kMcItems;
typedef unsigned long long u64;

struct McGrid {
    const float* sdf;
    int64_t sx, sy, sz;     // element strides of skimage's axes (x, y, z)
    int nx, ny, nz;
    int64_t n;              // nx * ny * nz; point p = (x * ny + y) * nz + z
};

__device__ __forceinline__ float mc_at(const McGrid& g, int x, int y, int z) {
    return g.sdf[(int64_t)x * g.sx + (int64_t)y * g.sy + (int64_t)z * g.sz];
}

// The point's three owned edges (crossing mask, bit a = edge along axis a) and, if it is a cell origin, the cell's case.
struct McPoint {
    float v, vn[3];
    int mask, cas;          // cas = -1: no cell
};

__device__ __forceinline__ McPoint mc_point(const McGrid& g, int64_t p, bool want_case) {
    McPoint q;
    const int z = (int)(p % g.nz);
    const int64_t r = p / g.nz;
    const int y = (int)(r % g.ny), x = (int)(r / g.ny);
    const bool ix = x + 1 < g.nx, iy = y + 1 < g.ny, iz = z + 1 < g.nz;
    q.v = mc_at(g, x, y, z);
    q.vn[0] = ix ? mc_at(g, x + 1, y, z) : q.v;
    q.vn[1] = iy ? mc_at(g, x, y + 1, z) : q.v;
    q.vn[2] = iz ? mc_at(g, x, y, z + 1) : q.v;
    const bool s = q.v > 0.0f;
    q.mask = ((q.vn[0] > 0.0f) != s ? 1 : 0) | ((q.vn[1] > 0.0f) != s ? 2 : 0) | ((q.vn[2] > 0.0f) != s ? 4 : 0);
    q.cas = -1;
    if (want_case && ix && iy && iz) {
        const float v3 = mc_at(g, x + 1, y + 1, z), v5 = mc_at(g, x + 1, y, z + 1), v6 = mc_at(g, x, y + 1, z + 1),
                    v7 = mc_at(g, x + 1, y + 1, z + 1);
        q.cas = (s ? 1 : 0) | (q.vn[0] > 0.0f ? 2 : 0) | (q.vn[1] > 0.0f ? 4 : 0) | (v3 > 0.0f ? 8 : 0) |
                (q.vn[2] > 0.0f ? 16 : 0) | (v5 > 0.0f ? 32 : 0) | (v6 > 0.0f ? 64 : 0) | (v7 > 0.0f ? 128 : 0);
    }
    return q;
}

// Exclusive scan over a 256-thread block (integer adds: the result does not depend on the order).  `lds`: 4 words; on return the
// block is synchronised and `lds` may be reused.
template <typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* lds, T& total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    T inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const T up = __shfl_up(inc, o, kWave);
        if (lane >= o) inc += up;
    }
    if (lane == kWave - 1) lds[wave] = inc;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kMcThreads / kWave; ++w) {
        const T s = lds[w];
        base += w < wave ? s : (T)0;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return base + inc - v;
}

__global__ void __launch_bounds__(kMcThreads)
mc_count_kernel(McGrid g, u64* __restrict__ bsum, int* __restrict__ bflag) {
    __shared__ u64 lds[kMcThreads / kWave];
    const int64_t base = (int64_t)blockIdx.x * kMcTile;
    u64 acc = 0;
    int le = 0, ge = 0;
    for (int k = 0; k < kMcItems; ++k) {
        const int64_t p = base + k * kMcThreads + threadIdx.x;
        if (p < g.n) {
            const McPoint q = mc_point(g, p, true);
            acc += (u64)__popc(q.mask) | ((u64)(q.cas >= 0 ? kMcTables.n_tris[q.cas] : 0) << 32);
            le |= !(q.v > 0.0f);            // NaN sets both: skimage's min / max comparisons are then false, no range error
            ge |= !(q.v < 0.0f);
        }
    }
    u64 tot;
    block_exclusive_scan(acc, lds, tot);
    le = __syncthreads_or(le);
    ge = __syncthreads_or(ge);
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = tot;
        bflag[blockIdx.x] = (le ? 1 : 0) | (ge ? 2 : 0);
    }
}

__global__ void __launch_bounds__(kMcThreads)
mc_scan_kernel(const u64* __restrict__ bsum, const int* __restrict__ bflag, u64* __restrict__ boff, int nblk, int* __restrict__ totals) {
    __shared__ u64 lds[kMcThreads / kWave];
    u64 carry = 0;
    int flags = 0;
    for (int b0 = 0; b0 < nblk; b0 += kMcThreads) {
        const int b = b0 + threadIdx.x;
        const u64 v = b < nblk ? bsum[b] : 0;
        u64 tot;
        const u64 ex = block_exclusive_scan(v, lds, tot);
        if (b < nblk) {
            boff[b] = carry + ex;
            flags |= bflag[b];
        }
        carry += tot;
    }
    const int le = __syncthreads_or(flags & 1), ge = __syncthreads_or(flags & 2);
    if (threadIdx.x == 0) {
        int nv = (int)(carry & 0xffffffffull), nf = (int)(carry >> 32);
        if (nv == 0 && !(le && ge)) nv = nf = -1;      // 0 outside [min, max]: skimage's ValueError
        totals[0] = nv;
        totals[1] = nf;
    }
}

// skimage's vertex on the edge from a (at index i) to b: float32(i + t), t = (0 - a) / (b - a) in double; then the reference's fp32
// transform (v / n - 0.5) * 0.24, negated on y and z.
__device__ __forceinline__ float mc_coord(int i, float a, float b, bool cross, int n, bool scene, bool negate) {
    float c = (float)i;
    if (cross) c = (float)((double)i + (0.0 - (double)a) / ((double)b - (double)a));
    if (!scene) return c;
    c = __fmul_rn(__fsub_rn(__fdiv_rn(c, (float)n), 0.5f), 0.24f);
    return negate ? -c : c;
}

__global__ void __launch_bounds__(kMcThreads)
mc_vertex_kernel(McGrid g, const u64* __restrict__ boff, unsigned* __restrict__ vinfo, float* __restrict__ verts, int64_t n_verts,
                 int scene) {
    __shared__ unsigned lds[kMcThreads / kWave];
    const int64_t base = (int64_t)blockIdx.x * kMcTile;
    unsigned carry = (unsigned)(boff[blockIdx.x] & 0xffffffffull);
    for (int k = 0; k < kMcItems; ++k) {
        const int64_t p = base + k * kMcThreads + threadIdx.x;
        McPoint q;
        q.mask = 0;
        if (p < g.n) q = mc_point(g, p, false);
        unsigned tot;
        const unsigned off = carry + block_exclusive_scan((unsigned)__popc(q.mask), lds, tot);
        carry += tot;
        if (p >= g.n) continue;
        vinfo[p] = (off << 3) | (unsigned)q.mask;
        if (!q.mask) continue;
        const int z = (int)(p % g.nz);
        const int64_t r = p / g.nz;
        const int y = (int)(r % g.ny), x = (int)(r / g.ny);
        int64_t o = off;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!((q.mask >> a) & 1)) continue;
            if (o < n_verts) {
                float* __restrict__ dst = verts + o * 3;
                dst[0] = mc_coord(x, q.v, q.vn[0], a == 0, g.nx, scene, false);
                dst[1] = mc_coord(y, q.v, q.vn[1], a == 1, g.ny, scene, true);
                dst[2] = mc_coord(z, q.v, q.vn[2], a == 2, g.nz, scene, true);
            }
            ++o;
        }
    }
}

__global__ void __launch_bounds__(kMcThreads)
mc_face_kernel(McGrid g, const u64* __restrict__ boff, const unsigned* __restrict__ vinfo, int* __restrict__ faces, int64_t n_faces) {
    __shared__ unsigned lds[kMcThreads / kWave];
    const int64_t base = (int64_t)blockIdx.x * kMcTile;
    unsigned carry = (unsigned)(boff[blockIdx.x] >> 32);
    const int64_t syx = (int64_t)g.ny * g.nz;
    for (int k = 0; k < kMcItems; ++k) {
        const int64_t p = base + k * kMcThreads + threadIdx.x;
        int cas = -1;
        if (p < g.n) cas = mc_point(g, p, true).cas;
        const int nt = cas >= 0 ? kMcTables.n_tris[cas] : 0;
        unsigned tot;
        const unsigned off = carry + block_exclusive_scan((unsigned)nt, lds, tot);
        carry += tot;
        for (int t = 0; t < nt; ++t) {
            if ((int64_t)off + t >= n_faces) break;
            int* __restrict__ dst = faces + ((int64_t)off + t) * 3;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int e = kMcTables.tri[cas][t][j], axis = e >> 2, jj = e & 3;
                // owner corner of edge e: offsets on the two other axes from jj (lower axis first)
                const int dx = axis == 0 ? 0 : (jj & 1);
                const int dy = axis == 1 ? 0 : (axis == 0 ? (jj & 1) : (jj >> 1));
                const int dz = axis == 2 ? 0 : (jj >> 1);
                const unsigned info = vinfo[p + dx * syx + dy * g.nz + dz];
                dst[j] = (int)((info >> 3) + __popc(info & ((1u << axis) - 1u)));
            }
        }
    }
}

struct McWorkspace {
    unsigned* vinfo;
    u64* bsum;
    u64* boff;
    int* bflag;
};

constexpr int64_t mc_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

int64_t mc_ws_bytes(int64_t n) {
    const int64_t nblk = (n + kMcTile - 1) / kMcTile;
    return mc_align(n * 4) + 2 * mc_align(nblk * 8) + mc_align(nblk * 4);
}

McWorkspace mc_ws(void* ws, int64_t n) {
    const int64_t nblk = (n + kMcTile - 1) / kMcTile;
    char* b = static_cast<char*>(ws);
    McWorkspace w;
    w.vinfo = reinterpret_cast<unsigned*>(b);
    b += mc_align(n * 4);
    w.bsum = reinterpret_cast<u64*>(b);
    b += mc_align(nblk * 8);
    w.boff = reinterpret_cast<u64*>(b);
    b += mc_align(nblk * 8);
    w.bflag = reinterpret_cast<int*>(b);
    return w;
}

// The largest grid: every count and packed offset stays inside its 32-bit field (at most 3 vertices and kMcMaxTris faces per point,
// vertex offsets shifted left by 3 in vinfo).
constexpr int64_t kMcMaxPoints = ((int64_t)1 << 31) / kMcMaxTris - 1;

int mc_check_sizes(int nx, int ny, int nz) {
    E3DGE_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "marching_cubes: the volume must be at least 2x2x2 (got %d x %d x %d)", nx, ny, nz);
    E3DGE_REQUIRE((int64_t)nx * ny * nz <= kMcMaxPoints, "marching_cubes: %d x %d x %d points exceed the 32-bit offsets (at most %lld)",
                  nx, ny, nz, (long long)kMcMaxPoints);
    return E3DGE_OK;
}

}  // namespace e3dge

using namespace e3dge;

extern "C" int64_t e3dge_marching_cubes_ws_bytes(int nx, int ny, int nz) {
    if (mc_check_sizes(nx, ny, nz) != E3DGE_OK) return -1;
    return mc_ws_bytes((int64_t)nx * ny * nz);
}

extern "C" int e3dge_marching_cubes_count(int* totals, void* ws, int64_t ws_bytes, const float* sdf, int nx, int ny, int nz, int64_t sx,
                                          int64_t sy, int64_t sz, e3dge_stream_t stream) {
    const int rc = mc_check_sizes(nx, ny, nz);
    if (rc != E3DGE_OK) return rc;
    E3DGE_REQUIRE(totals && ws && sdf, "marching_cubes_count: null pointer");
    const int64_t n = (int64_t)nx * ny * nz;
    E3DGE_REQUIRE(ws_bytes >= mc_ws_bytes(n), "marching_cubes_count: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
                  (long long)mc_ws_bytes(n));
    const McGrid g{sdf, sx, sy, sz, nx, ny, nz, n};
    const McWorkspace w = mc_ws(ws, n);
    const int nblk = (int)((n + kMcTile - 1) / kMcTile);
    mc_count_kernel<<<dim3(nblk), dim3(kMcThreads), 0, as_stream(stream)>>>(g, w.bsum, w.bflag);
    int e = check_launch("marching_cubes_count");
    if (e != E3DGE_OK) return e;
    mc_scan_kernel<<<dim3(1), dim3(kMcThreads), 0, as_stream(stream)>>>(w.bsum, w.bflag, w.boff, nblk, totals);
    return check_launch("marching_cubes_scan");
}

extern "C" int e3dge_marching_cubes_emit(float* verts, int* faces, int64_t n_verts, int64_t n_faces, const void* ws, int64_t ws_bytes,
                                         const float* sdf, int nx, int ny, int nz, int64_t sx, int64_t sy, int64_t sz, int scene,
                                         e3dge_stream_t stream) {
    const int rc = mc_check_sizes(nx, ny, nz);
    if (rc != E3DGE_OK) return rc;
    E3DGE_REQUIRE(ws && sdf, "marching_cubes_emit: null pointer");
    E3DGE_REQUIRE(n_verts >= 0 && n_faces >= 0 && (n_verts == 0 || verts) && (n_faces == 0 || faces),
                  "marching_cubes_emit: null output or negative count");
    const int64_t n = (int64_t)nx * ny * nz;
    E3DGE_REQUIRE(ws_bytes >= mc_ws_bytes(n), "marching_cubes_emit: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
                  (long long)mc_ws_bytes(n));
    const McGrid g{sdf, sx, sy, sz, nx, ny, nz, n};
    McWorkspace w = mc_ws(const_cast<void*>(ws), n);
    const int nblk = (int)((n + kMcTile - 1) / kMcTile);
    mc_vertex_kernel<<<dim3(nblk), dim3(kMcThreads), 0, as_stream(stream)>>>(g, w.boff, w.vinfo, verts, n_verts, scene ? 1 : 0);
    int e = check_launch("marching_cubes_vertices");
    if (e != E3DGE_OK) return e;
    mc_face_kernel<<<dim3(nblk), dim3(kMcThreads), 0, as_stream(stream)>>>(g, w.boff, w.vinfo, faces, n_faces);
    return check_launch("marching_cubes_faces");
}

extern "C" int e3dge_marching_cubes_tables(int* n_tris, int* tri_edges) {
    E3DGE_REQUIRE(n_tris && tri_edges, "marching_cubes_tables: null pointer");
    for (int c = 0; c < 256; ++c) {
        n_tris[c] = kMcHostTables.n_tris[c];
        for (int t = 0; t < kMcMaxTris; ++t)
            for (int j = 0; j < 3; ++j)
                tri_edges[(c * kMcMaxTris + t) * 3 + j] = t < kMcHostTables.n_tris[c] ? kMcHostTables.tri[c][t][j] : -1;
    }
    return E3DGE_OK;
}
