// Surface renderings: the depth mesh of an xyz map, angle-weighted vertex normals, and a tiled mesh rasteriser with Phong shading and
// soft blending in one kernel.
//
// Reference: xyz2mesh (project/utils/mesh_utils.py:107-126), trimesh's vertex_normals and the pytorch3d renderer of create_mesh_renderer
// (mesh_utils.py:145-173: MeshRasterizer + SoftPhongShader) as AERunner.render_depth_mesh / render_trimesh drive them
// (project/trainers/trainer.py:2254-2346, 1482-1534).  The contract, the face order and the spelling of every formula are in
// include/e3dge_hip.h next to e3dge_mesh_render; DESIGN.md 4.12c has the kernels, the bound and the measured times.
//
// depth mesh   one launch: thread p = r w + c writes vertex p and the two triangles of cell (r, c).
// normals      faces: per face the unit normal and the three corner angles in float64, added to the vertices' accumulators as 2^40
//              fixed-point int64 (integer adds commute: the sums do not depend on the order the atomics arrive in); vertices: the sum,
//              normalised.
// render       vertices: view and NDC coordinates once per vertex -> faces: culling, pixel bounding box, per-tile counts -> scan (one
//              block) -> fill: face indices into the per-tile lists (slot order is arbitrary; the K-list's tie rule makes the result
//              independent of it) -> raster: one 256-thread workgroup per 16 x 16-pixel tile, one pixel per thread (each wave an 8 x 16
//              pixel block), face records staged through LDS 256 at a time and read by broadcast, the K nearest fragments of a pixel in
//              registers (K a template parameter), shading and blending at the end of the same kernel.
// noise        the reference's NoiseInjection.project_noise (project/models/stylesdf_model.py:365-466): the same binning stages and
//              fragment walk at K = 17, blending up to four scalar vertex fields instead of a Phong colour.
// subdivide    midpoint subdivision (trimesh.remesh.subdivide), one launch per level; the caller ranks the edge keys.
#include "common.h"

namespace e3dge {

constexpr int kMrThreads = 256, kMrTile = 16;
constexpr int kMrEmpty = 0x7fffffff;
typedef unsigned long long mr_u64;

constexpr int64_t mr_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

// ---- depth mesh ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kMrThreads)
depth_mesh_kernel(float* __restrict__ verts, int* __restrict__ faces, const float* __restrict__ xyz, int h, int w) {
    const int64_t n = (int64_t)h * w;
    const int64_t p = (int64_t)blockIdx.x * kMrThreads + threadIdx.x;
    if (p >= n) return;
    verts[p * 3 + 0] = xyz[p];
    verts[p * 3 + 1] = xyz[n + p];
    verts[p * 3 + 2] = xyz[2 * n + p];
    const int r = (int)(p / w), c = (int)(p % w);
    if (r + 1 < h && c + 1 < w) {
        int* __restrict__ f = faces + ((int64_t)r * (w - 1) + c) * 6;
        const int a = (int)p, b = (int)p + w;
        f[0] = a;
        f[1] = b;
        f[2] = a + 1;
        f[3] = b;
        f[4] = b + 1;
        f[5] = a + 1;
    }
}

// ---- vertex normals -------------------------------------------------------------------------------------------------------------------------
constexpr double kVnScale = 1099511627776.0;      // 2^40: |angle * n| <= pi, so a vertex may collect 2^21 faces before int64 overflows

__device__ __forceinline__ double vn_corner_angle(const double* a, const double* b) {      // a, b unit vectors
    double d = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    d = d < -1.0 ? -1.0 : d > 1.0 ? 1.0 : d;
    return acos(d);
}

__global__ void __launch_bounds__(kMrThreads)
vn_face_kernel(mr_u64* __restrict__ acc, const float* __restrict__ verts, const int* __restrict__ faces, int64_t n_verts, int64_t n_faces) {
    const int64_t f = (int64_t)blockIdx.x * kMrThreads + threadIdx.x;
    if (f >= n_faces) return;
    int idx[3];
    double v[3][3];
    for (int k = 0; k < 3; ++k) {
        idx[k] = faces[f * 3 + k];
        if (idx[k] < 0 || idx[k] >= n_verts) return;
    }
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) v[k][a] = (double)verts[(int64_t)idx[k] * 3 + a];
    double e[3][3], len[3];                        // e[k] = unit vector from corner k to corner k + 1
    for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3;
        for (int a = 0; a < 3; ++a) e[k][a] = v[k1][a] - v[k][a];
        len[k] = sqrt(e[k][0] * e[k][0] + e[k][1] * e[k][1] + e[k][2] * e[k][2]);
    }
    double n[3] = {e[0][1] * -e[2][2] - e[0][2] * -e[2][1], e[0][2] * -e[2][0] - e[0][0] * -e[2][2],
                   e[0][0] * -e[2][1] - e[0][1] * -e[2][0]};           // (v1 - v0) x (v2 - v0)
    const double nl = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(nl > 0.0) || !(len[0] > 0.0) || !(len[1] > 0.0) || !(len[2] > 0.0)) return;      // degenerate (or NaN): contributes nothing
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) e[k][a] /= len[k];
    for (int a = 0; a < 3; ++a) n[a] /= nl;
    for (int k = 0; k < 3; ++k) {
        const int kp = (k + 2) % 3;
        const double back[3] = {-e[kp][0], -e[kp][1], -e[kp][2]};
        const double ang = vn_corner_angle(e[k], back);
        if (!(ang == ang)) return;
        for (int a = 0; a < 3; ++a)
            atomicAdd(acc + (int64_t)idx[k] * 3 + a, (mr_u64)(long long)llrint(ang * n[a] * kVnScale));
    }
}

__global__ void __launch_bounds__(kMrThreads)
vn_vertex_kernel(float* __restrict__ normals, const mr_u64* __restrict__ acc, int64_t n_verts) {
    const int64_t i = (int64_t)blockIdx.x * kMrThreads + threadIdx.x;
    if (i >= n_verts) return;
    double s[3];
    for (int a = 0; a < 3; ++a) s[a] = (double)(long long)acc[i * 3 + a];
    const double l = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    for (int a = 0; a < 3; ++a) normals[i * 3 + a] = l > 0.0 ? (float)(s[a] / l) : 0.0f;
}

// ---- mesh rendering ---------------------------------------------------------------------------------------------------------------------------
struct MrParams {
    float cam[12];
    float t, znear, zfar;
    float light[3], ambient[3], diffuse[3], specular[3], background[3];
    float blur, sigma, gamma;
    int S, tiles;                   // tiles per image side
};

// A vertex after the vertex pass.  NDC in float64: what the edge functions are sensitive to is the position relative to a face's size, and
// a face on the silhouette is 1e-4 NDC wide with a depth range that is not small.
struct alignas(8) MrVert {
    double x, y;                    // NDC
    float z;                        // view space
    int pad;
};

struct MrWorkspace {
    MrVert* vcache;
    int2* ftile;                    // per face: tile ranges (x0 | x1 << 16, y0 | y1 << 16); x0 > x1: culled
    unsigned* count;                // per tile
    unsigned* offset;
    unsigned* cursor;
    int* entries;
};

int64_t mr_ws_bytes(int64_t nv, int64_t nf, int64_t n_tiles, int64_t cap) {
    return mr_align(nv * (int64_t)sizeof(MrVert)) + mr_align(nf * 8) + 3 * mr_align(n_tiles * 4) + mr_align(cap * 4);
}

MrWorkspace mr_ws(void* ws, int64_t nv, int64_t nf, int64_t n_tiles) {
    char* b = static_cast<char*>(ws);
    MrWorkspace w;
    w.vcache = reinterpret_cast<MrVert*>(b);
    b += mr_align(nv * (int64_t)sizeof(MrVert));
    w.ftile = reinterpret_cast<int2*>(b);
    b += mr_align(nf * 8);
    w.count = reinterpret_cast<unsigned*>(b);
    b += mr_align(n_tiles * 4);
    w.offset = reinterpret_cast<unsigned*>(b);
    b += mr_align(n_tiles * 4);
    w.cursor = reinterpret_cast<unsigned*>(b);
    b += mr_align(n_tiles * 4);
    w.entries = reinterpret_cast<int*>(b);
    return w;
}

__global__ void __launch_bounds__(kMrThreads)
mr_vertex_kernel(MrParams P, MrVert* __restrict__ vcache, const float* __restrict__ verts, int64_t n_verts) {
    const int64_t i = (int64_t)blockIdx.x * kMrThreads + threadIdx.x;
    if (i >= n_verts) return;
    const double dx = (double)verts[i * 3 + 0] - P.cam[0], dy = (double)verts[i * 3 + 1] - P.cam[1], dz = (double)verts[i * 3 + 2] - P.cam[2];
    const double vx = dx * P.cam[3] + dy * P.cam[4] + dz * P.cam[5];
    const double vy = dx * P.cam[6] + dy * P.cam[7] + dz * P.cam[8];
    const double vz = dx * P.cam[9] + dy * P.cam[10] + dz * P.cam[11];
    const double den = vz * P.t;
    MrVert v;
    v.x = vx / den;
    v.y = vy / den;
    v.z = (float)vz;
    v.pad = 0;
    vcache[i] = v;
}

__device__ __forceinline__ double mr_area(const MrVert& a, const MrVert& b, const MrVert& c) {
    return (c.x - a.x) * (b.y - a.y) - (c.y - a.y) * (b.x - a.x);
}

// Pixel index of an NDC coordinate, as a float: centre j sits at 1 - (2 j + 1) / S.
__device__ __forceinline__ float mr_pixel_of(float ndc, int S) { return ((1.0f - ndc) * (float)S - 1.0f) * 0.5f; }

// The face's candidate test and its range of tiles; false: culled.
__device__ __forceinline__ bool mr_face_tiles(const MrParams& P, const int* __restrict__ faces, const MrVert* __restrict__ vcache,
                                              int64_t f, int64_t n_verts, int& tx0, int& tx1, int& ty0, int& ty1) {
    const int i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= n_verts || i1 >= n_verts || i2 >= n_verts) return false;
    const MrVert a = vcache[i0], b = vcache[i1], c = vcache[i2];
    const float zc = P.znear * 0.5f;
    if (!(a.z >= zc) || !(b.z >= zc) || !(c.z >= zc)) return false;
    if (!(fabs(mr_area(a, b, c)) > 1e-8)) return false;
    const float r = sqrtf(P.blur), last = (float)(P.S - 1);
    const float ax = (float)a.x, ay = (float)a.y, bx = (float)b.x, by = (float)b.y, cx = (float)c.x, cy = (float)c.y;
    const float xmin = fminf(ax, fminf(bx, cx)) - r, xmax = fmaxf(ax, fmaxf(bx, cx)) + r;
    const float ymin = fminf(ay, fminf(by, cy)) - r, ymax = fmaxf(ay, fmaxf(by, cy)) + r;
    // one pixel wider than the box on both sides: the raster kernel tests the widened NDC box itself
    const float jlo = floorf(mr_pixel_of(xmax, P.S)) - 1.0f, jhi = ceilf(mr_pixel_of(xmin, P.S)) + 1.0f;
    const float ilo = floorf(mr_pixel_of(ymax, P.S)) - 1.0f, ihi = ceilf(mr_pixel_of(ymin, P.S)) + 1.0f;
    if (!(jhi >= 0.0f) || !(jlo <= last) || !(ihi >= 0.0f) || !(ilo <= last)) return false;
    tx0 = (int)fminf(fmaxf(jlo, 0.0f), last) / kMrTile;
    tx1 = (int)fminf(fmaxf(jhi, 0.0f), last) / kMrTile;
    ty0 = (int)fminf(fmaxf(ilo, 0.0f), last) / kMrTile;
    ty1 = (int)fminf(fmaxf(ihi, 0.0f), last) / kMrTile;
    return tx0 <= tx1 && ty0 <= ty1;
}

__global__ void __launch_bounds__(kMrThreads)
mr_face_kernel(MrParams P, int2* __restrict__ ftile, unsigned* __restrict__ count, const int* __restrict__ faces,
               const MrVert* __restrict__ vcache, int64_t n_verts, int64_t n_faces) {
    const int64_t f = (int64_t)blockIdx.x * kMrThreads + threadIdx.x;
    if (f >= n_faces) return;
    int tx0 = 1, tx1 = 0, ty0 = 1, ty1 = 0;
    if (!mr_face_tiles(P, faces, vcache, f, n_verts, tx0, tx1, ty0, ty1)) {
        ftile[f] = make_int2(1, 1);                 // x0 = 1 > x1 = 0
        return;
    }
    ftile[f] = make_int2(tx0 | (tx1 << 16), ty0 | (ty1 << 16));
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) atomicAdd(count + ty * P.tiles + tx, 1u);
}

// One block: exclusive scan of the tile counts; status = {entries needed, capacity}.  Carry = unsigned: the totals fit 32 bits by the
// caller's check (faces x tiles < 2^31).  Carry = mr_u64 (noise projection: no such bound): `entries needed` saturates at 2^31 - 1 --
// above every capacity the entry accepts -- and so do the offsets, so that offset + cursor neither wraps nor passes the fill's guard.
template <typename Carry>
__global__ void __launch_bounds__(kMrThreads)
mr_scan_kernel(const unsigned* __restrict__ count, unsigned* __restrict__ offset, int n_tiles, int* __restrict__ status, int capacity) {
    __shared__ Carry lds[kMrThreads / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    Carry carry = 0;
    for (int b0 = 0; b0 < n_tiles; b0 += kMrThreads) {
        const int b = b0 + threadIdx.x;
        const Carry v = b < n_tiles ? count[b] : 0u;
        Carry inc = v;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const Carry up = __shfl_up(inc, o, kWave);
            if (lane >= o) inc += up;
        }
        if (lane == kWave - 1) lds[wave] = inc;
        __syncthreads();
        Carry base = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kMrThreads / kWave; ++w) {
            const Carry s = lds[w];
            base += w < wave ? s : (Carry)0;
            tot += s;
        }
        __syncthreads();
        if (b < n_tiles) {
            const Carry o = carry + base + inc - v;
            if constexpr (sizeof(Carry) == 8) offset[b] = (unsigned)(o < (Carry)0x7fffffff ? o : (Carry)0x7fffffff);
            else offset[b] = o;
        }
        carry += tot;
    }
    if (threadIdx.x == 0) {
        if constexpr (sizeof(Carry) == 8) status[0] = (int)(carry < (Carry)0x7fffffff ? carry : (Carry)0x7fffffff);
        else status[0] = (int)carry;
        status[1] = capacity;
    }
}

__global__ void __launch_bounds__(kMrThreads)
mr_fill_kernel(int tiles, const int2* __restrict__ ftile, const unsigned* __restrict__ offset, unsigned* __restrict__ cursor,
               int* __restrict__ entries, int64_t n_faces, int capacity) {
    const int64_t f = (int64_t)blockIdx.x * kMrThreads + threadIdx.x;
    if (f >= n_faces) return;
    const int2 t = ftile[f];
    const int tx0 = t.x & 0xffff, tx1 = t.x >> 16, ty0 = t.y & 0xffff, ty1 = t.y >> 16;
    if (tx0 > tx1) return;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const int tile = ty * tiles + tx;
            const unsigned slot = offset[tile] + atomicAdd(cursor + tile, 1u);
            if (slot < (unsigned)capacity) entries[slot] = (int)f;
        }
}

// A face as the raster loop reads it from LDS (five 16-byte reads, every lane the same address).
struct alignas(16) MrRecord {
    double x0, y0, x1, y1, x2, y2;  // NDC
    float z0, z1, z2;               // view space
    int face;
    float bx0, bx1, by0, by1;       // the NDC bounding box widened by sqrt(blur_radius)
};

// Squared distance from q to the segment a-b (pytorch3d's PointLineDistanceForward).
__device__ __forceinline__ float mr_seg_d2(float qx, float qy, float ax, float ay, float bx, float by) {
    const float ex = bx - ax, ey = by - ay;
    const float l2 = ex * ex + ey * ey;
    if (l2 <= 1e-8f) return (qx - bx) * (qx - bx) + (qy - by) * (qy - by);
    const float t = fminf(fmaxf((ex * (qx - ax) + ey * (qy - ay)) / l2, 0.0f), 1.0f);
    const float px = ax + t * ex, py = ay + t * ey;
    return (qx - px) * (qx - px) + (qy - py) * (qy - py);
}

// Screen barycentrics of q; true when all three are positive.  float64 from the vertex pass to the fragment's depth: differences and
// products of the coordinates are then free of the cancellation that costs a thin face its depth in float32.
__device__ __forceinline__ bool mr_bary(const MrRecord& r, float qxf, float qyf, double& w0, double& w1, double& w2) {
    const double qx = qxf, qy = qyf;
    const double inv = 1.0 / ((r.x2 - r.x0) * (r.y1 - r.y0) - (r.y2 - r.y0) * (r.x1 - r.x0));
    w0 = ((qx - r.x1) * (r.y2 - r.y1) - (qy - r.y1) * (r.x2 - r.x1)) * inv;
    w1 = ((qx - r.x2) * (r.y0 - r.y2) - (qy - r.y2) * (r.x0 - r.x2)) * inv;
    w2 = ((qx - r.x0) * (r.y1 - r.y0) - (qy - r.y0) * (r.x1 - r.x0)) * inv;
    return w0 > 0.0 && w1 > 0.0 && w2 > 0.0;
}

// Perspective-correct, clipped barycentrics (in place) and the fragment's view-space depth.
__device__ __forceinline__ float mr_persp_clip(const MrRecord& r, double& w0, double& w1, double& w2) {
    const double z0 = r.z0, z1 = r.z1, z2 = r.z2;
    const double t0 = w0 / z0, t1 = w1 / z1, t2 = w2 / z2;
    const double inv = 1.0 / (t0 + t1 + t2);
    w0 = fmin(fmax(t0 * inv, 0.0), 1.0);
    w1 = fmin(fmax(t1 * inv, 0.0), 1.0);
    w2 = fmin(fmax(t2 * inv, 0.0), 1.0);
    const double s = 1.0 / fmax(w0 + w1 + w2, 1e-5);
    w0 *= s;
    w1 *= s;
    w2 *= s;
    return (float)(w0 * z0 + w1 * z1 + w2 * z2);
}

__device__ __forceinline__ MrRecord mr_record(const MrVert& a, const MrVert& b, const MrVert& c, int face, float blur) {
    MrRecord r;
    r.x0 = a.x; r.y0 = a.y; r.x1 = b.x; r.y1 = b.y; r.x2 = c.x; r.y2 = c.y;
    r.z0 = a.z; r.z1 = b.z; r.z2 = c.z;
    r.face = face;
    const float w = sqrtf(blur);
    const float ax = (float)a.x, ay = (float)a.y, bx = (float)b.x, by = (float)b.y, cx = (float)c.x, cy = (float)c.y;
    r.bx0 = fminf(ax, fminf(bx, cx)) - w;
    r.bx1 = fmaxf(ax, fmaxf(bx, cx)) + w;
    r.by0 = fminf(ay, fminf(by, cy)) - w;
    r.by1 = fmaxf(ay, fmaxf(by, cy)) + w;
    return r;
}

__device__ __forceinline__ void mr_normalize(float& x, float& y, float& z) {
    const float l = fmaxf(sqrtf(x * x + y * y + z * z), 1e-6f);
    x /= l;
    y /= l;
    z /= l;
}

// The K nearest covered fragments of pixel centre (qx, qy) among the faces of `tile`, ordered by (z, face index): lz / ld / lf, empty
// slots (inf, 0, kMrEmpty).  Every thread of the workgroup calls it (face records are staged through `rec` 256 at a time); threads
// that are not `live` only stage.  The insertion is unrolled over K: every index into the three arrays is a compile-time constant, so
// they stay in registers (a runtime index would move them to scratch).
template <int K>
__device__ __forceinline__ void mr_nearest_fragments(const MrParams& P, MrRecord* rec, int tile, bool live, float qx, float qy,
                                                     const unsigned* __restrict__ count, const unsigned* __restrict__ offset,
                                                     const int* __restrict__ entries, const int* __restrict__ faces,
                                                     const MrVert* __restrict__ vcache, float (&lz)[K], float (&ld)[K], int (&lf)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        lz[k] = __builtin_inff();
        ld[k] = 0.0f;
        lf[k] = kMrEmpty;
    }
    const unsigned n = count[tile], base = offset[tile];
    for (unsigned c0 = 0; c0 < n; c0 += kMrThreads) {
        const unsigned m = min(n - c0, (unsigned)kMrThreads);
        if (threadIdx.x < m) {
            const int f = entries[base + c0 + threadIdx.x];
            rec[threadIdx.x] = mr_record(vcache[faces[(int64_t)f * 3]], vcache[faces[(int64_t)f * 3 + 1]],
                                         vcache[faces[(int64_t)f * 3 + 2]], f, P.blur);
        }
        __syncthreads();
        if (live) {
            for (unsigned s = 0; s < m; ++s) {
                const MrRecord& r = rec[s];
                if (qx < r.bx0 || qx > r.bx1 || qy < r.by0 || qy > r.by1) continue;
                double w0, w1, w2;
                const bool inside = mr_bary(r, qx, qy, w0, w1, w2);
                const float x0 = (float)r.x0, y0 = (float)r.y0, x1 = (float)r.x1, y1 = (float)r.y1, x2 = (float)r.x2, y2 = (float)r.y2;
                const float d2 = fminf(mr_seg_d2(qx, qy, x0, y0, x1, y1), fminf(mr_seg_d2(qx, qy, x1, y1, x2, y2), mr_seg_d2(qx, qy, x2, y2, x0, y0)));
                if (!inside && !(d2 < P.blur)) continue;
                float cz = mr_persp_clip(r, w0, w1, w2);
                if (!(cz >= 0.0f)) continue;
                float cd = inside ? -d2 : d2;
                int cf = r.face;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (cz < lz[k] || (cz == lz[k] && cf < lf[k])) {
                        const float tz = lz[k], td = ld[k];
                        const int tf = lf[k];
                        lz[k] = cz; ld[k] = cd; lf[k] = cf;
                        cz = tz; cd = td; cf = tf;
                    }
                }
            }
        }
        __syncthreads();
    }
}

template <int K>
__global__ void __launch_bounds__(kMrThreads)
mr_raster_kernel(MrParams P, const int* __restrict__ status, const unsigned* __restrict__ count, const unsigned* __restrict__ offset,
                 const int* __restrict__ entries, const int* __restrict__ faces, const MrVert* __restrict__ vcache,
                 const float* __restrict__ verts, const float* __restrict__ normals, const float* __restrict__ colors,
                 float* __restrict__ image, float* __restrict__ zbuf, int* __restrict__ pix_to_face) {
    __shared__ MrRecord rec[kMrThreads];
    if (status[0] > status[1]) return;              // the lists did not fit: the caller reads status and launches again
    const int tile = blockIdx.x, tx = tile % P.tiles, ty = tile / P.tiles;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int j = tx * kMrTile + (lane & 7) + 8 * (wave & 1), i = ty * kMrTile + (lane >> 3) + 8 * (wave >> 1);
    const bool live = i < P.S && j < P.S;
    const float qx = 1.0f - (float)(2 * j + 1) / (float)P.S, qy = 1.0f - (float)(2 * i + 1) / (float)P.S;

    float lz[K], ld[K];
    int lf[K];
    mr_nearest_fragments<K>(P, rec, tile, live, qx, qy, count, offset, entries, faces, vcache, lz, ld, lf);
    if (!live) return;

    const int64_t pix = (int64_t)i * P.S + j;
    float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f, keep = 1.0f;
    const float range = P.zfar - P.znear;
    const float m_raw = (P.zfar - lz[0]) / range;               // the largest zi: lz[0] is the nearest kept fragment
    const bool clamped = !(m_raw >= 1e-10f);
    const float m = clamped ? 1e-10f : m_raw;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const bool have = lf[k] != kMrEmpty;
        zbuf[pix * K + k] = have ? lz[k] : -1.0f;
        pix_to_face[pix * K + k] = have ? lf[k] : -1;
        if (!have) continue;
        const int64_t f = lf[k];
        const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
        const MrRecord r = mr_record(vcache[i0], vcache[i1], vcache[i2], (int)f, P.blur);
        double b0, b1, b2;
        mr_bary(r, qx, qy, b0, b1, b2);
        mr_persp_clip(r, b0, b1, b2);
        const float w0 = (float)b0, w1 = (float)b1, w2 = (float)b2;
        float pos[3], nrm[3], tex[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            pos[a] = w0 * verts[(int64_t)i0 * 3 + a] + w1 * verts[(int64_t)i1 * 3 + a] + w2 * verts[(int64_t)i2 * 3 + a];
            nrm[a] = w0 * normals[(int64_t)i0 * 3 + a] + w1 * normals[(int64_t)i1 * 3 + a] + w2 * normals[(int64_t)i2 * 3 + a];
            tex[a] = colors ? w0 * colors[(int64_t)i0 * 3 + a] + w1 * colors[(int64_t)i1 * 3 + a] + w2 * colors[(int64_t)i2 * 3 + a] : 1.0f;
        }
        mr_normalize(nrm[0], nrm[1], nrm[2]);
        float lx = P.light[0] - pos[0], ly = P.light[1] - pos[1], lzz = P.light[2] - pos[2];
        mr_normalize(lx, ly, lzz);
        const float c = nrm[0] * lx + nrm[1] * ly + nrm[2] * lzz;
        float vx = P.cam[0] - pos[0], vy = P.cam[1] - pos[1], vz = P.cam[2] - pos[2];
        mr_normalize(vx, vy, vz);
        const float rx = 2.0f * c * nrm[0] - lx, ry = 2.0f * c * nrm[1] - ly, rz = 2.0f * c * nrm[2] - lzz;
        float sp = c > 0.0f ? fmaxf(vx * rx + vy * ry + vz * rz, 0.0f) : 0.0f;
#pragma unroll
        for (int q = 0; q < 6; ++q) sp *= sp;                                   // shininess 64
        const float diff = fmaxf(c, 0.0f);
        const float prob = 1.0f / (1.0f + expf(-(-ld[k] / P.sigma)));
        const float e = clamped ? (P.zfar - lz[k]) / range - m : (lz[0] - lz[k]) / range;
        const float w = prob * expf(e / P.gamma);
#pragma unroll
        for (int a = 0; a < 3; ++a) num[a] += w * ((P.ambient[a] + P.diffuse[a] * diff) * tex[a] + P.specular[a] * sp);
        den += w;
        keep *= 1.0f - prob;
    }
    if (lf[0] == kMrEmpty) {
#pragma unroll
        for (int a = 0; a < 3; ++a) image[pix * 4 + a] = P.background[a];
        image[pix * 4 + 3] = 0.0f;
        return;
    }
    const float delta = fmaxf(expf((1e-10f - m) / P.gamma), 1e-10f);
#pragma unroll
    for (int a = 0; a < 3; ++a) image[pix * 4 + a] = (num[a] + delta * P.background[a]) / (den + delta);
    image[pix * 4 + 3] = 1.0f - keep;
}

template <int K>
int mr_launch_raster(const MrParams& P, const E3dgeMeshRenderArgs& a, const MrWorkspace& w, hipStream_t stream) {
    mr_raster_kernel<K><<<dim3(P.tiles * P.tiles), dim3(kMrThreads), 0, stream>>>(
        P, a.status, w.count, w.offset, w.entries, a.faces, w.vcache, a.verts, a.normals, a.colors, a.image, a.zbuf, a.pix_to_face);
    return check_launch("mesh_render_raster");
}

// ---- noise projection ------------------------------------------------------------------------------------------------------------------
// The rasteriser's fragment walk at K = 17, then the blend of up to four scalar vertex fields that share the rasterisation (the
// decoder's noise maps of one size): colour = the interpolated field, ambient 1, no diffuse or specular term, background 1.  Per pixel
// 3 x 17 registers of (z, d, face); the texels are read at the end, once per kept fragment.
constexpr int kNpK = E3DGE_NOISE_PROJECT_FACES_PER_PIXEL, kNpMaxMaps = E3DGE_NOISE_PROJECT_MAX_MAPS;

__global__ void __launch_bounds__(kMrThreads)
np_raster_kernel(MrParams P, const int* __restrict__ status, const unsigned* __restrict__ count, const unsigned* __restrict__ offset,
                 const int* __restrict__ entries, const int* __restrict__ faces, const MrVert* __restrict__ vcache,
                 const float* __restrict__ vert_noise, int64_t n_verts, int n_maps, const float* __restrict__ prev,
                 float* __restrict__ out, unsigned char* __restrict__ valid) {
    __shared__ MrRecord rec[kMrThreads];
    if (status[0] > status[1]) return;              // the lists did not fit: the caller reads status and launches again
    const int tile = blockIdx.x, tx = tile % P.tiles, ty = tile / P.tiles;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int j = tx * kMrTile + (lane & 7) + 8 * (wave & 1), i = ty * kMrTile + (lane >> 3) + 8 * (wave >> 1);
    const bool live = i < P.S && j < P.S;
    const float qx = 1.0f - (float)(2 * j + 1) / (float)P.S, qy = 1.0f - (float)(2 * i + 1) / (float)P.S;

    float lz[kNpK], ld[kNpK];
    int lf[kNpK];
    mr_nearest_fragments<kNpK>(P, rec, tile, live, qx, qy, count, offset, entries, faces, vcache, lz, ld, lf);
    if (!live) return;

    const int64_t pix = (int64_t)i * P.S + j, plane = (int64_t)P.S * P.S;
    float num[kNpMaxMaps] = {0.0f, 0.0f, 0.0f, 0.0f}, den = 0.0f, zmax = -1.0f;
    const float range = P.zfar - P.znear;
    const float m_raw = (P.zfar - lz[0]) / range;
    const bool clamped = !(m_raw >= 1e-10f);
    const float m = clamped ? 1e-10f : m_raw;
#pragma unroll
    for (int k = 0; k < kNpK; ++k) {
        if (lf[k] == kMrEmpty) continue;
        const int64_t f = lf[k];
        const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
        const MrRecord r = mr_record(vcache[i0], vcache[i1], vcache[i2], (int)f, P.blur);
        double b0, b1, b2;
        mr_bary(r, qx, qy, b0, b1, b2);
        mr_persp_clip(r, b0, b1, b2);
        const float w0 = (float)b0, w1 = (float)b1, w2 = (float)b2;
        const float prob = 1.0f / (1.0f + expf(-(-ld[k] / P.sigma)));
        const float e = clamped ? (P.zfar - lz[k]) / range - m : (lz[0] - lz[k]) / range;
        const float w = prob * expf(e / P.gamma);
#pragma unroll
        for (int c = 0; c < kNpMaxMaps; ++c) {
            if (c < n_maps) {
                const float* __restrict__ vn = vert_noise + c * n_verts;
                num[c] += w * (w0 * vn[i0] + w1 * vn[i1] + w2 * vn[i2]);
            }
        }
        den += w;
        zmax = fmaxf(zmax, lz[k]);
    }
    const bool ok = zmax > 0.0f;                    // the reference's zbuf.max(-1) > 0
    valid[pix] = ok ? 1 : 0;
    const float delta = fmaxf(expf((1e-10f - m) / P.gamma), 1e-10f);
#pragma unroll
    for (int c = 0; c < kNpMaxMaps; ++c)
        if (c < n_maps) out[c * plane + pix] = ok ? (num[c] + delta) / (den + delta) : prev[c * plane + pix];
}

// ---- midpoint subdivision ----------------------------------------------------------------------------------------------------------------
// One launch: thread i copies vertex i (i < V), writes the midpoint of edge i - V (V <= i < V + E) and the four faces of face i (i < F).
__global__ void __launch_bounds__(kMrThreads)
subdivide_kernel(float* __restrict__ out_verts, int* __restrict__ out_faces, const float* __restrict__ verts, const int* __restrict__ faces,
                 const int64_t* __restrict__ edge_keys, const int* __restrict__ side_rank, int64_t n_verts, int64_t n_faces, int64_t n_edges) {
    const int64_t i = (int64_t)blockIdx.x * kMrThreads + threadIdx.x;
    if (i < n_verts) {
        for (int a = 0; a < 3; ++a) out_verts[i * 3 + a] = verts[i * 3 + a];
    } else if (i < n_verts + n_edges) {
        const int64_t key = edge_keys[i - n_verts];
        const int64_t lo = key / n_verts, hi = key % n_verts;
        const bool ok = key >= 0 && lo < n_verts;      // a key that is no vertex pair: a vertex at the origin, nothing read
        for (int a = 0; a < 3; ++a) out_verts[i * 3 + a] = ok ? 0.5f * (verts[lo * 3 + a] + verts[hi * 3 + a]) : 0.0f;
    }
    if (i < n_faces) {
        const int a = faces[i * 3], b = faces[i * 3 + 1], c = faces[i * 3 + 2];
        const int ab = (int)n_verts + side_rank[i * 3], bc = (int)n_verts + side_rank[i * 3 + 1], ca = (int)n_verts + side_rank[i * 3 + 2];
        int* __restrict__ o = out_faces + i * 12;
        o[0] = a;  o[1] = ab;  o[2] = ca;
        o[3] = ab; o[4] = b;   o[5] = bc;
        o[6] = ca; o[7] = bc;  o[8] = c;
        o[9] = ab; o[10] = bc; o[11] = ca;
    }
}

constexpr int kMrMaxSize = 16384;                   // tile indices are packed into 16 bits

int mr_check_sizes(const char* what, int64_t n_verts, int64_t n_faces, int image_size, int64_t bin_capacity, bool narrow) {
    E3DGE_REQUIRE(n_verts >= 0 && n_faces >= 0 && n_verts < ((int64_t)1 << 31) && n_faces < ((int64_t)1 << 31),
                  "%s: %lld vertices, %lld faces", what, (long long)n_verts, (long long)n_faces);
    E3DGE_REQUIRE(image_size >= 1 && image_size <= kMrMaxSize, "%s: image_size %d outside 1..%d", what, image_size, kMrMaxSize);
    const int64_t t = (image_size + kMrTile - 1) / kMrTile;
    // narrow: 32-bit totals in the scan; otherwise the scan carries 64 bits and saturates at 2^31 - 1, which no capacity reaches
    E3DGE_REQUIRE(!narrow || n_faces * t * t < ((int64_t)1 << 31), "%s: %lld faces x %lld tiles exceed the 32-bit bin offsets", what,
                  (long long)n_faces, (long long)(t * t));
    E3DGE_REQUIRE(bin_capacity >= 0 && bin_capacity < ((int64_t)1 << 31) - (narrow ? 0 : 1), "%s: bin capacity %lld", what, (long long)bin_capacity);
    return E3DGE_OK;
}

// vertices -> faces -> scan -> fill: the per-tile face lists both raster kernels read.
template <typename Carry>
int mr_bin_faces(const MrParams& P, const MrWorkspace& w, const float* verts, const int* faces, int64_t n_verts, int64_t n_faces,
                 int64_t n_tiles, int* status, int64_t bin_capacity, hipStream_t s) {
    // count, offset and cursor are adjacent: one clear
    if (hipMemsetAsync(w.count, 0, (size_t)(3 * mr_align(n_tiles * 4)), s) != hipSuccess) return check_launch("mesh_render_clear");
    int e;
    if (n_verts > 0) {
        mr_vertex_kernel<<<dim3((unsigned)((n_verts + kMrThreads - 1) / kMrThreads)), dim3(kMrThreads), 0, s>>>(P, w.vcache, verts, n_verts);
        if ((e = check_launch("mesh_render_vertices")) != E3DGE_OK) return e;
    }
    const unsigned fblocks = (unsigned)((n_faces + kMrThreads - 1) / kMrThreads);
    if (n_faces > 0) {
        mr_face_kernel<<<dim3(fblocks), dim3(kMrThreads), 0, s>>>(P, w.ftile, w.count, faces, w.vcache, n_verts, n_faces);
        if ((e = check_launch("mesh_render_faces")) != E3DGE_OK) return e;
    }
    mr_scan_kernel<Carry><<<dim3(1), dim3(kMrThreads), 0, s>>>(w.count, w.offset, (int)n_tiles, status, (int)bin_capacity);
    if ((e = check_launch("mesh_render_scan")) != E3DGE_OK) return e;
    if (n_faces > 0) {
        mr_fill_kernel<<<dim3(fblocks), dim3(kMrThreads), 0, s>>>(P.tiles, w.ftile, w.offset, w.cursor, w.entries, n_faces, (int)bin_capacity);
        if ((e = check_launch("mesh_render_fill")) != E3DGE_OK) return e;
    }
    return E3DGE_OK;
}

}  // namespace e3dge

using namespace e3dge;

extern "C" int e3dge_depth_mesh(float* verts, int32_t* faces, const float* xyz, int h, int w, e3dge_stream_t stream) {
    E3DGE_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31), "depth_mesh: a %d x %d map", h, w);
    E3DGE_REQUIRE(verts && xyz && (faces || h == 1 || w == 1), "depth_mesh: null pointer");
    const int64_t n = (int64_t)h * w;
    depth_mesh_kernel<<<dim3((unsigned)((n + kMrThreads - 1) / kMrThreads)), dim3(kMrThreads), 0, as_stream(stream)>>>(verts, faces, xyz, h, w);
    return check_launch("depth_mesh");
}

extern "C" int64_t e3dge_vertex_normals_ws_bytes(int64_t n_verts) {
    if (n_verts < 0 || n_verts >= ((int64_t)1 << 31)) return -1;
    return mr_align(n_verts * 3 * 8);
}

extern "C" int e3dge_vertex_normals(float* normals, const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, void* ws,
                                    int64_t ws_bytes, e3dge_stream_t stream) {
    E3DGE_REQUIRE(n_verts >= 0 && n_faces >= 0 && n_verts < ((int64_t)1 << 31) && n_faces < ((int64_t)1 << 31),
                  "vertex_normals: %lld vertices, %lld faces", (long long)n_verts, (long long)n_faces);
    E3DGE_REQUIRE((n_verts == 0 || (normals && verts && ws)) && (n_faces == 0 || faces), "vertex_normals: null pointer");
    E3DGE_REQUIRE(ws_bytes >= e3dge_vertex_normals_ws_bytes(n_verts), "vertex_normals: workspace of %lld bytes, %lld needed",
                  (long long)ws_bytes, (long long)e3dge_vertex_normals_ws_bytes(n_verts));
    if (n_verts == 0) return E3DGE_OK;
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(ws, 0, (size_t)(n_verts * 3 * 8), s) != hipSuccess) return check_launch("vertex_normals_clear");
    mr_u64* acc = static_cast<mr_u64*>(ws);
    if (n_faces > 0) {
        vn_face_kernel<<<dim3((unsigned)((n_faces + kMrThreads - 1) / kMrThreads)), dim3(kMrThreads), 0, s>>>(acc, verts, faces, n_verts, n_faces);
        const int e = check_launch("vertex_normals_faces");
        if (e != E3DGE_OK) return e;
    }
    vn_vertex_kernel<<<dim3((unsigned)((n_verts + kMrThreads - 1) / kMrThreads)), dim3(kMrThreads), 0, s>>>(normals, acc, n_verts);
    return check_launch("vertex_normals_vertices");
}

extern "C" int64_t e3dge_mesh_render_ws_bytes(int64_t n_verts, int64_t n_faces, int image_size, int64_t bin_capacity) {
    if (mr_check_sizes("mesh_render", n_verts, n_faces, image_size, bin_capacity, true) != E3DGE_OK) return -1;
    const int64_t t = (image_size + kMrTile - 1) / kMrTile;
    return mr_ws_bytes(n_verts, n_faces, t * t, bin_capacity);
}

extern "C" int e3dge_mesh_render(const E3dgeMeshRenderArgs* args, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "mesh_render: null args");
    const E3dgeMeshRenderArgs& a = *args;
    const int rc = mr_check_sizes("mesh_render", a.n_verts, a.n_faces, a.image_size, a.bin_capacity, true);
    if (rc != E3DGE_OK) return rc;
    E3DGE_REQUIRE(a.faces_per_pixel >= 1 && a.faces_per_pixel <= E3DGE_MESH_MAX_FACES_PER_PIXEL, "mesh_render: faces_per_pixel %d outside 1..%d",
                  a.faces_per_pixel, E3DGE_MESH_MAX_FACES_PER_PIXEL);
    E3DGE_REQUIRE(a.image && a.zbuf && a.pix_to_face && a.status && a.ws, "mesh_render: null output, status or workspace");
    E3DGE_REQUIRE((a.n_verts == 0 || (a.verts && a.normals)) && (a.n_faces == 0 || a.faces), "mesh_render: null mesh pointer");
    E3DGE_REQUIRE(a.tan_half_fov > 0.0f && a.zfar > a.znear && a.znear > 0.0f && a.blur_radius >= 0.0f && a.sigma > 0.0f && a.gamma > 0.0f,
                  "mesh_render: tan_half_fov, znear < zfar, sigma and gamma must be positive, blur_radius non-negative");
    const int64_t t = (a.image_size + kMrTile - 1) / kMrTile, n_tiles = t * t;
    const int64_t need = mr_ws_bytes(a.n_verts, a.n_faces, n_tiles, a.bin_capacity);
    E3DGE_REQUIRE(a.ws_bytes >= need, "mesh_render: workspace of %lld bytes, %lld needed", (long long)a.ws_bytes, (long long)need);
    MrParams P;
    for (int k = 0; k < 12; ++k) P.cam[k] = a.camera[k];
    P.t = a.tan_half_fov; P.znear = a.znear; P.zfar = a.zfar;
    for (int k = 0; k < 3; ++k) {
        P.light[k] = a.light_location[k];
        P.ambient[k] = a.ambient_color[k];
        P.diffuse[k] = a.diffuse_color[k];
        P.specular[k] = a.specular_color[k];
        P.background[k] = a.background_color[k];
    }
    P.blur = a.blur_radius; P.sigma = a.sigma; P.gamma = a.gamma;
    P.S = a.image_size; P.tiles = (int)t;
    const MrWorkspace w = mr_ws(a.ws, a.n_verts, a.n_faces, n_tiles);
    hipStream_t s = as_stream(stream);
    const int e = mr_bin_faces<unsigned>(P, w, a.verts, a.faces, a.n_verts, a.n_faces, n_tiles, a.status, a.bin_capacity, s);
    if (e != E3DGE_OK) return e;
    switch (a.faces_per_pixel) {
        case 1: return mr_launch_raster<1>(P, a, w, s);
        case 2: return mr_launch_raster<2>(P, a, w, s);
        case 3: return mr_launch_raster<3>(P, a, w, s);
        case 4: return mr_launch_raster<4>(P, a, w, s);
        case 5: return mr_launch_raster<5>(P, a, w, s);
        case 6: return mr_launch_raster<6>(P, a, w, s);
        case 7: return mr_launch_raster<7>(P, a, w, s);
        default: return mr_launch_raster<8>(P, a, w, s);
    }
}

extern "C" int64_t e3dge_noise_project_ws_bytes(int64_t n_verts, int64_t n_faces, int image_size, int64_t bin_capacity) {
    if (mr_check_sizes("noise_project", n_verts, n_faces, image_size, bin_capacity, false) != E3DGE_OK) return -1;
    const int64_t t = (image_size + kMrTile - 1) / kMrTile;
    return mr_ws_bytes(n_verts, n_faces, t * t, bin_capacity);
}

extern "C" int e3dge_noise_project(const E3dgeNoiseProjectArgs* args, e3dge_stream_t stream) {
    E3DGE_REQUIRE(args, "noise_project: null args");
    const E3dgeNoiseProjectArgs& a = *args;
    const int rc = mr_check_sizes("noise_project", a.n_verts, a.n_faces, a.image_size, a.bin_capacity, false);
    if (rc != E3DGE_OK) return rc;
    E3DGE_REQUIRE(a.n_maps >= 1 && a.n_maps <= E3DGE_NOISE_PROJECT_MAX_MAPS, "noise_project: n_maps %d outside 1..%d", a.n_maps,
                  E3DGE_NOISE_PROJECT_MAX_MAPS);
    E3DGE_REQUIRE(a.out && a.valid && a.prev && a.status && a.ws, "noise_project: null output, prev, status or workspace");
    E3DGE_REQUIRE((a.n_verts == 0 || (a.verts && a.vert_noise)) && (a.n_faces == 0 || a.faces), "noise_project: null mesh pointer");
    E3DGE_REQUIRE(a.tan_half_fov > 0.0f && a.zfar > a.znear && a.znear > 0.0f && a.blur_radius >= 0.0f && a.sigma > 0.0f && a.gamma > 0.0f,
                  "noise_project: tan_half_fov, znear < zfar, sigma and gamma must be positive, blur_radius non-negative");
    const int64_t t = (a.image_size + kMrTile - 1) / kMrTile, n_tiles = t * t;
    const int64_t need = mr_ws_bytes(a.n_verts, a.n_faces, n_tiles, a.bin_capacity);
    E3DGE_REQUIRE(a.ws_bytes >= need, "noise_project: workspace of %lld bytes, %lld needed", (long long)a.ws_bytes, (long long)need);
    MrParams P = {};
    for (int k = 0; k < 12; ++k) P.cam[k] = a.camera[k];
    P.t = a.tan_half_fov; P.znear = a.znear; P.zfar = a.zfar;
    P.blur = a.blur_radius; P.sigma = a.sigma; P.gamma = a.gamma;
    P.S = a.image_size; P.tiles = (int)t;
    const MrWorkspace w = mr_ws(a.ws, a.n_verts, a.n_faces, n_tiles);
    hipStream_t s = as_stream(stream);
    const int e = mr_bin_faces<mr_u64>(P, w, a.verts, a.faces, a.n_verts, a.n_faces, n_tiles, a.status, a.bin_capacity, s);
    if (e != E3DGE_OK) return e;
    np_raster_kernel<<<dim3((unsigned)n_tiles), dim3(kMrThreads), 0, s>>>(P, a.status, w.count, w.offset, w.entries, a.faces, w.vcache, a.vert_noise,
                                                                          a.n_verts, a.n_maps, a.prev, a.out, a.valid);
    return check_launch("noise_project_raster");
}

extern "C" int e3dge_mesh_subdivide(float* out_verts, int32_t* out_faces, const float* verts, const int32_t* faces, const int64_t* edge_keys,
                                    const int32_t* side_rank, int64_t n_verts, int64_t n_faces, int64_t n_edges, e3dge_stream_t stream) {
    E3DGE_REQUIRE(n_verts >= 0 && n_faces >= 0 && n_edges >= 0 && n_edges <= 3 * n_faces && n_verts + n_edges < ((int64_t)1 << 31) &&
                      4 * n_faces < ((int64_t)1 << 31),
                  "mesh_subdivide: %lld vertices, %lld faces, %lld edges", (long long)n_verts, (long long)n_faces, (long long)n_edges);
    E3DGE_REQUIRE((n_verts == 0 || (out_verts && verts)) && (n_faces == 0 || (out_faces && faces && side_rank)) && (n_edges == 0 || edge_keys),
                  "mesh_subdivide: null pointer");
    E3DGE_REQUIRE(n_edges == 0 || n_verts > 0, "mesh_subdivide: edges without vertices");
    const int64_t n = n_verts + n_edges > n_faces ? n_verts + n_edges : n_faces;
    if (n == 0) return E3DGE_OK;
    subdivide_kernel<<<dim3((unsigned)((n + kMrThreads - 1) / kMrThreads)), dim3(kMrThreads), 0, as_stream(stream)>>>(
        out_verts, out_faces, verts, faces, edge_keys, side_rank, n_verts, n_faces, n_edges);
    return check_launch("mesh_subdivide");
}
