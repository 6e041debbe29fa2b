// Signed distance from many points to a triangle mesh, brute force (the rule in full: include/tpgan_ops.h, "signed
// distance to a triangle mesh"; the numpy statement: tests/mesh_sdf_rule.py).
//
// Launch shape.  One thread per query, 256 per workgroup, grid ceil(Q / 256).  The triangles pass through LDS in tiles of
// 256: thread t of the workgroup stages triangle tile + t -- its three fp32 corners, and for the sign its corners snapped
// to the integer grid, the integer normal, the yz bounding box of its projection and the ownership bits of its three
// projected edges, all of which depend on the triangle alone.  In the loop over a tile every lane reads the SAME LDS
// address (a broadcast: no bank conflicts).  The magnitude is the region form of the closest point with selects in place
// of branches; the sign rejects on the integer yz box first (one branch, mostly uniform: a triangle's projection is small)
// and only then evaluates the three 64-bit edge functions and the determinant.  A running (d2, face) minimum with a strict
// comparison over ascending faces is the minimum with ties to the lowest face whatever the tiling.  No atomics, no
// scratch; 32 KiB of LDS.
//
// fp32 operations are + - * / and sqrtf only, each rounded on its own (-ffp-contract=off); the sign is integer arithmetic
// whose every intermediate stays below 6 * 2^48.
#include "tpg_common.hpp"

namespace {

constexpr int MS_TILE = 256;
constexpr int MS_MAX = 1 << 30;              // Q, V, F: 3 * index stays far inside 64 bits, the grid inside 2^23 blocks
constexpr float MS_GRID = 65536.0f;

struct __attribute__((aligned(16))) MsTri {
    float ax, ay, az, bx;
    float by, bz, cx, cy;
    float cz;
    int valid;                               // fp32 normal not exactly zero
    int ymin, ymax;                          // the projection's integer box; empty (1, 0) where the sign skips the triangle
    int zmin, zmax, iax, iay;
    int iaz, iby, ibz, icy;                  // B and C already exchanged where the projected area was negative
    int icz, own, pad0, pad1;                // own: bit e set iff edge e owns the points on it
    long long nx, ny;                        // integer normal of the (exchanged) corners: nx > 0
    long long nz, pad2;
};
static_assert(sizeof(MsTri) == 128, "eight 16-byte reads per triangle");

struct MsBox { float lo[3], hi[3]; };

// q = floor((x - origin) * inv_unit + 0.5), clamped into [0, 2^16] (NaN: 0)
__device__ __forceinline__ int ms_snap(float x, float origin, float inv_unit) {
    float t = floorf((x - origin) * inv_unit + 0.5f);
    t = t >= 0.0f ? t : 0.0f;
    t = t <= MS_GRID ? t : MS_GRID;
    return (int)t;
}

__device__ __forceinline__ float ms_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

// an edge U -> V of a positively oriented projection owns the points on it iff its direction lies in the half-open
// half-plane dy > 0 or (dy == 0 and dz > 0)
__device__ __forceinline__ int ms_owns(int uy, int uz, int vy, int vz) {
    const int dy = vy - uy, dz = vz - uz;
    return (dy > 0 || (dy == 0 && dz > 0)) ? 1 : 0;
}

__device__ __forceinline__ long long ms_edge(int uy, int uz, int vy, int vz, int py, int pz) {
    return (long long)(vy - uy) * (pz - uz) - (long long)(vz - uz) * (py - uy);
}

__global__ __launch_bounds__(256) void mesh_sdf_kernel(const float *__restrict__ query, const float *__restrict__ vertices,
                                                       const int32_t *__restrict__ faces, int Q, int V, int F, MsBox box,
                                                       float inv_unit, float *__restrict__ dist,
                                                       int32_t *__restrict__ face) {
    __shared__ MsTri tile[MS_TILE];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * 256 + tid;
    const bool live = i < Q;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (live) px = query[i * 3], py = query[i * 3 + 1], pz = query[i * 3 + 2];
    const bool inbox = px >= box.lo[0] && px <= box.hi[0] && py >= box.lo[1] && py <= box.hi[1] && pz >= box.lo[2] &&
                       pz <= box.hi[2];
    const int qx = inbox ? ms_snap(px, box.lo[0], inv_unit) : 0;
    const int qy = inbox ? ms_snap(py, box.lo[1], inv_unit) : 0;
    const int qz = inbox ? ms_snap(pz, box.lo[2], inv_unit) : 0;
    float best = __builtin_inff();
    int best_f = -1;
    unsigned crossings = 0;

    for (int f0 = 0; f0 < F; f0 += MS_TILE) {
        const int nt = min(MS_TILE, F - f0);
        __syncthreads();                                   // the tile before has been read by every lane
        if (tid < nt) {
            const size_t fr = (size_t)(f0 + tid) * 3;
            // a true clamp (a negative index is vertex 0), as the rule states it
            const size_t ia = (size_t)min(max(faces[fr], 0), V - 1) * 3, ib = (size_t)min(max(faces[fr + 1], 0), V - 1) * 3,
                         ic = (size_t)min(max(faces[fr + 2], 0), V - 1) * 3;
            MsTri t;
            t.ax = vertices[ia], t.ay = vertices[ia + 1], t.az = vertices[ia + 2];
            t.bx = vertices[ib], t.by = vertices[ib + 1], t.bz = vertices[ib + 2];
            t.cx = vertices[ic], t.cy = vertices[ic + 1], t.cz = vertices[ic + 2];
            const float ux = t.bx - t.ax, uy = t.by - t.ay, uz = t.bz - t.az;
            const float vx = t.cx - t.ax, vy = t.cy - t.ay, vz = t.cz - t.az;
            const float fnx = uy * vz - uz * vy, fny = uz * vx - ux * vz, fnz = ux * vy - uy * vx;
            t.valid = !(fnx == 0.0f && fny == 0.0f && fnz == 0.0f);
            const int Ax = ms_snap(t.ax, box.lo[0], inv_unit), Ay = ms_snap(t.ay, box.lo[1], inv_unit),
                      Az = ms_snap(t.az, box.lo[2], inv_unit);
            int Bx = ms_snap(t.bx, box.lo[0], inv_unit), By = ms_snap(t.by, box.lo[1], inv_unit),
                Bz = ms_snap(t.bz, box.lo[2], inv_unit);
            int Cx = ms_snap(t.cx, box.lo[0], inv_unit), Cy = ms_snap(t.cy, box.lo[1], inv_unit),
                Cz = ms_snap(t.cz, box.lo[2], inv_unit);
            const long long area = (long long)(By - Ay) * (Cz - Az) - (long long)(Bz - Az) * (Cy - Ay);
            if (area < 0) {
                int s;
                s = Bx, Bx = Cx, Cx = s;
                s = By, By = Cy, Cy = s;
                s = Bz, Bz = Cz, Cz = s;
            }
            t.nx = (long long)(By - Ay) * (Cz - Az) - (long long)(Bz - Az) * (Cy - Ay);
            t.ny = (long long)(Bz - Az) * (Cx - Ax) - (long long)(Bx - Ax) * (Cz - Az);
            t.nz = (long long)(Bx - Ax) * (Cy - Ay) - (long long)(By - Ay) * (Cx - Ax);
            const bool counts = t.valid && area != 0;
            t.ymin = counts ? min(Ay, min(By, Cy)) : 1;
            t.ymax = counts ? max(Ay, max(By, Cy)) : 0;
            t.zmin = min(Az, min(Bz, Cz));
            t.zmax = max(Az, max(Bz, Cz));
            t.iax = Ax, t.iay = Ay, t.iaz = Az, t.iby = By, t.ibz = Bz, t.icy = Cy, t.icz = Cz;
            t.own = ms_owns(By, Bz, Cy, Cz) | (ms_owns(Cy, Cz, Ay, Az) << 1) | (ms_owns(Ay, Az, By, Bz) << 2);
            t.pad0 = t.pad1 = 0;
            t.pad2 = 0;
            tile[tid] = t;
        }
        __syncthreads();
        for (int k = 0; k < nt; ++k) {
            const MsTri &t = tile[k];
            // ---- the sign: does the ray in +x from (qx, qy, qz) cross this triangle strictly ahead
            if (inbox && qy >= t.ymin && qy <= t.ymax && qz >= t.zmin && qz <= t.zmax) {
                const long long e0 = ms_edge(t.iby, t.ibz, t.icy, t.icz, qy, qz);
                const long long e1 = ms_edge(t.icy, t.icz, t.iay, t.iaz, qy, qz);
                const long long e2 = ms_edge(t.iay, t.iaz, t.iby, t.ibz, qy, qz);
                const bool in = (e0 > 0 || (e0 == 0 && (t.own & 1))) && (e1 > 0 || (e1 == 0 && (t.own & 2))) &&
                                (e2 > 0 || (e2 == 0 && (t.own & 4)));
                const long long det = (t.nx * (qx - t.iax) + t.ny * (qy - t.iay)) + t.nz * (qz - t.iaz);
                crossings += (in && det < 0) ? 1u : 0u;
            }
            if (!t.valid) continue;                        // uniform
            // ---- the magnitude: the closest point of the triangle, region form
            const float abx = t.bx - t.ax, aby = t.by - t.ay, abz = t.bz - t.az;
            const float acx = t.cx - t.ax, acy = t.cy - t.ay, acz = t.cz - t.az;
            const float apx = px - t.ax, apy = py - t.ay, apz = pz - t.az;
            const float d1 = ms_dot(abx, aby, abz, apx, apy, apz), d2 = ms_dot(acx, acy, acz, apx, apy, apz);
            const float bpx = px - t.bx, bpy = py - t.by, bpz = pz - t.bz;
            const float d3 = ms_dot(abx, aby, abz, bpx, bpy, bpz), d4 = ms_dot(acx, acy, acz, bpx, bpy, bpz);
            const float cpx = px - t.cx, cpy = py - t.cy, cpz = pz - t.cz;
            const float d5 = ms_dot(abx, aby, abz, cpx, cpy, cpz), d6 = ms_dot(acx, acy, acz, cpx, cpy, cpz);
            const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
            const float e43 = d4 - d3, e56 = d5 - d6;
            // the face, then the regions from the last to the first in priority: the first that holds wins
            const float sum = (va + vb) + vc;
            float v = vb / sum, w = vc / sum;
            const bool rbc = va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f;
            const float wbc = e43 / (e43 + e56);
            v = rbc ? 1.0f - wbc : v, w = rbc ? wbc : w;
            const bool rac = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
            const float wac = d2 / (d2 - d6);
            v = rac ? 0.0f : v, w = rac ? wac : w;
            const bool rc = d6 >= 0.0f && d5 <= d6;
            v = rc ? 0.0f : v, w = rc ? 1.0f : w;
            const bool rab = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
            const float vab = d1 / (d1 - d3);
            v = rab ? vab : v, w = rab ? 0.0f : w;
            const bool rb = d3 >= 0.0f && d4 <= d3;
            v = rb ? 1.0f : v, w = rb ? 0.0f : w;
            const bool ra = d1 <= 0.0f && d2 <= 0.0f;
            v = ra ? 0.0f : v, w = ra ? 0.0f : w;
            // the closest point is a + v ab + w ac; its offset from the query
            const float rx = apx - (v * abx + w * acx), ry = apy - (v * aby + w * acy), rz = apz - (v * abz + w * acz);
            const float dd = (rx * rx + ry * ry) + rz * rz;
            const bool better = dd < best;
            best = better ? dd : best;
            best_f = better ? f0 + k : best_f;
        }
    }
    if (!live) return;
    const float d = sqrtf(best);
    dist[i] = (crossings & 1u) ? -d : d;                  // every triangle skipped: no crossing, +inf
    face[i] = best_f;
}

bool ms_finite(float v) { return v - v == 0.0f; }

}  // namespace

extern "C" int tpg_mesh_sdf_f32(const float *query, const float *vertices, const int32_t *faces, int Q, int V, int F,
                                const float *box, float inv_unit, float *dist, int32_t *face, void *stream) {
    if (!query || !vertices || !faces || !box || !dist || !face || Q < 0 || V < 0 || F < 0) return TPG_ERR_ARG;
    if (!ms_finite(inv_unit) || !(inv_unit > 0.0f)) return TPG_ERR_ARG;
    MsBox bx;
    for (int d = 0; d < 3; ++d) {
        bx.lo[d] = box[d], bx.hi[d] = box[3 + d];
        if (!ms_finite(bx.lo[d]) || !ms_finite(bx.hi[d]) || !(bx.lo[d] <= bx.hi[d])) return TPG_ERR_ARG;
    }
    if (Q == 0) return TPG_OK;
    if (F == 0 || V == 0 || Q > MS_MAX || V > MS_MAX || F > MS_MAX) return TPG_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(mesh_sdf_kernel, dim3((Q + 255) / 256), dim3(256), 0, tpg_stream(stream), query, vertices, faces, Q,
                       V, F, bx, inv_unit, dist, face);
    TPG_RETURN_IF_LAUNCH_FAILED();
    return TPG_OK;
}
