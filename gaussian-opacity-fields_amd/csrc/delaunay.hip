// delaunay.hip -- Delaunay tetrahedralization of a float32 point set (the reference's tetranerf `cpp.triangulate`, CGAL's
// Delaunay_triangulation_3, which extract_mesh.py runs on the Gaussians' tetra points).  Contract: DESIGN.md §3.7; ABI:
// include/gof_delaunay_hip.h.
//
// Parallel Bowyer-Watson insertion in rounds over a triangulation with an infinite vertex (1 finite + 4 infinite cells to start, as
// CGAL does): every live cell that holds uninserted points nominates one of them (dt_nominate), each nominee grows its conflict
// cavity by a walk across faces (perturbed in-sphere test), claims its cavity cells and the cells across the cavity's boundary with
// an atomicMin of its priority (a hash of the point); nominees that hold all claims after the kernel boundary win and replace their
// cavity by one cell per boundary face.  The smallest claimant always wins, so every round inserts a point.  The smallest nominee
// whose cavity outgrew the per-nominee slot is grown by one thread (the slow path) and claims with priority 0, so it wins as well.
//
// Cells: verts[c] = 4 vertex ids (DT_INF = infinite vertex), positively oriented (det[v1-v0, v2-v0, v3-v0] > 0; for a cell with the
// infinite vertex: positive once the infinite vertex is replaced by a point beyond its finite face).  nbr[c][i] = 4 * cell + face of
// the neighbour across the face opposite verts[c][i].  kill[c] = the point whose insertion deleted c (DT_NONE: live).
// Points: the distinct input points, sorted along a Morton curve; pt_cell[q] = the cell an uninserted point q is assigned to:
// a finite cell that contains it (closed), or an infinite cell it conflicts with.
#include <algorithm>
#include <cstring>
#include "gof_common.h"
#include "radix.h"
#include "gof_geom.h"
#include "delaunay_predicates.h"
#include "../../include/gof_delaunay_hip.h"

namespace gof {

using dt::Pred;

constexpr uint32_t DT_INF = 0xFFFFFFFFu;       // the infinite vertex
constexpr uint32_t DT_NONE = 0xFFFFFFFFu;
constexpr uint32_t PT_DONE = 0xFFFFFFFFu;      // pt_cell: inserted (or one of the start points)
constexpr uint32_t PT_LOST = 0xFFFFFFFEu;      // pt_cell: no new cell of the inserting point took it (located by a global scan)
constexpr int DT_FAST_CELLS = 128;             // cavity cells of a fast-path slot
constexpr int DT_FAST_FACES = 256;             // boundary faces of a fast-path slot
constexpr int DT_SLOT_WORDS = 4 + DT_FAST_CELLS + DT_FAST_FACES;
constexpr int64_t DT_MAX_CELLS = (int64_t)1 << 30;   // nbr packs 4 * cell + face into 32 bits
constexpr int DT_MAX_ROUNDS = 1 << 20;
constexpr int DT_THREADS = 256;
constexpr int DT_DIRS = 256;                  // directions of the extreme points (dt_extremes)

// error bits of the header
constexpr uint32_t DTE_EXPANSION = 1u, DTE_ORIENT = 2u, DTE_LOCATE = 4u, DTE_WALK = 8u, DTE_CAPACITY = 16u, DTE_PERTURB = 32u;

// the device header (first 256 bytes of the workspace); words read back once per round
struct DtHeader {
    uint32_t ncells;        // cells in the arena (live + dead)
    uint32_t err;           // DTE_* bits
    uint32_t winners;       // fast-path winners of the round
    uint32_t need;          // cells the winners create
    uint32_t nslots;        // nominating cells this round (may exceed the slot count)
    uint32_t bigmin;        // smallest nominee whose cavity outgrew its slot
    uint32_t slow_done;     // the slow path inserted a point
    uint32_t slow_nc, slow_nf;   // the slow-path nominee's cavity cells / boundary faces (0: none this round)
    uint32_t nonfinite;     // an input coordinate is not finite
    uint32_t start[4];      // the 4 start points (DT_NONE: not found)
    uint32_t ndistinct;
    uint32_t live;          // live cells after a compaction / finite live cells at the end
    uint32_t lost;          // points located by the global scan (statistics)
    uint32_t bbox[6];       // orderable keys: min x y z, max x y z
    uint32_t active;        // which cell buffer is active (written by the host)
    uint32_t pad0;
    long long n, cap;       // the build's point count and cell capacity (the workspace layout)
    unsigned long long exact;   // exact predicate evaluations
    long long stats[8];     // gof_delaunay_stats: rounds, exact, peak cells, slow insertions, lost, distinct, capacity, cells
};

struct DtWs {
    DtHeader* hdr;
    float* xyz;             // [n][3] distinct points, Morton order
    uint32_t* orig;         // [n] input index of each distinct point
    uint32_t* pt_cell;      // [n]
    uint32_t* newbase;      // [n] first new cell of an inserted point (this round)
    uint32_t* newcount;     // [n]
    uint32_t* key[2];       // [n] sort keys (dedup and Morton order)
    uint32_t* val[2];       // [n] sort values
    uint32_t* tmp;          // sort / scan scratch
    int4* verts[2];         // [cap] double buffer (the inactive one: slow-path cavity lists, emitted cells)
    uint4* nbr[2];          // [cap]
    uint32_t* claim;        // [cap]
    uint32_t* kill;         // [cap]
    unsigned long long* nominee;   // [cap] nominee_key of the cell's nominee
    uint32_t* map;          // [cap + 1]
    uint32_t* slots;        // [nslot][DT_SLOT_WORDS]
    int64_t n, cap, nslot;
};

static inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

static int64_t slot_count(int64_t n)
{
    int64_t s = n / 16;
    if (s < 256) s = 256;
    if (s > (1 << 18)) s = 1 << 18;
    return s;
}

template <class T>
static inline void carve(char*& p, T*& ptr, size_t count)
{
    ptr = reinterpret_cast<T*>(p);
    p += a256(count * sizeof(T));
}

static size_t dt_layout(int64_t n, int64_t cap, void* base, DtWs* w)
{
    DtWs o;
    char* p = (char*)base;
    const size_t m = (size_t)(n > cap ? n : cap);
    size_t tw = rs_tmp_words(m);
    if (scan_tmp_words((size_t)cap + 1) > tw) tw = scan_tmp_words((size_t)cap + 1);
    carve(p, o.hdr, 1);
    carve(p, o.xyz, 3 * (size_t)n);
    carve(p, o.orig, n);
    carve(p, o.pt_cell, n);
    carve(p, o.newbase, n);
    carve(p, o.newcount, n);
    for (int k = 0; k < 2; k++) { carve(p, o.key[k], n); carve(p, o.val[k], n); }     // (the emit's sort uses the inactive nbr buffer)
    carve(p, o.tmp, tw);
    for (int k = 0; k < 2; k++) { carve(p, o.verts[k], cap); carve(p, o.nbr[k], cap); }
    carve(p, o.claim, cap);
    carve(p, o.kill, cap);
    carve(p, o.nominee, cap);
    carve(p, o.map, cap + 1);
    o.nslot = slot_count(n);
    carve(p, o.slots, (size_t)o.nslot * DT_SLOT_WORDS);
    o.n = n;
    o.cap = cap;
    if (w) *w = o;
    return (size_t)(p - (char*)base);
}

static inline uint32_t blocks(int64_t n) { return (uint32_t)((n + DT_THREADS - 1) / DT_THREADS); }

// ---------------------------------------------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t vget(const int4& v, int i) { return (uint32_t)(i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w); }
__device__ __forceinline__ void vset(int4& v, int i, uint32_t x)
{
    if (i == 0) v.x = (int)x; else if (i == 1) v.y = (int)x; else if (i == 2) v.z = (int)x; else v.w = (int)x;
}
__device__ __forceinline__ uint32_t nget(const uint4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
__device__ __forceinline__ void nset(uint4& v, int i, uint32_t x)
{
    if (i == 0) v.x = x; else if (i == 1) v.y = x; else if (i == 2) v.z = x; else v.w = x;
}
__device__ __forceinline__ int vindex(const int4& v, uint32_t x)
{
    return vget(v, 0) == x ? 0 : vget(v, 1) == x ? 1 : vget(v, 2) == x ? 2 : 3;
}
__device__ __forceinline__ int inf_index(const int4& v)
{
    return vget(v, 0) == DT_INF ? 0 : vget(v, 1) == DT_INF ? 1 : vget(v, 2) == DT_INF ? 2 : vget(v, 3) == DT_INF ? 3 : -1;
}
// orientation of cell v with vertex k replaced by point p (all four finite after the replacement)
__device__ __forceinline__ int orient_rep(const Pred& P, int4 v, int k, uint32_t p)
{
    vset(v, k, p);
    return dt::orient(P, vget(v, 0), vget(v, 1), vget(v, 2), vget(v, 3));
}

// Perturbed in-sphere of a finite positive cell (Devillers-Teillaud, lexicographic order; CGAL's side_of_oriented_sphere with
// perturb = true): > 0 in conflict, < 0 not.  Never 0.
__device__ int insphere_perturbed(const Pred& P, const int4& v, uint32_t p, uint32_t* err)
{
    const int s = dt::insphere(P, vget(v, 0), vget(v, 1), vget(v, 2), vget(v, 3), p);
    if (s) return s;
    uint32_t id[5] = {vget(v, 0), vget(v, 1), vget(v, 2), vget(v, 3), p};
    int pos[5] = {0, 1, 2, 3, 4};
    for (int i = 1; i < 5; i++)              // ascending lexicographic order of the 5 points
        for (int j = i; j > 0 && dt::lex_less(P, id[pos[j]], id[pos[j - 1]]); j--) { const int t = pos[j]; pos[j] = pos[j - 1]; pos[j - 1] = t; }
    for (int i = 4; i > 1; i--) {
        const int k = pos[i];
        if (k == 4) return -1;
        const int o = orient_rep(P, v, k, p);
        if (o) return o;
    }
    atomicOr(err, DTE_PERTURB);
    return -1;
}

// Perturbed in-circle of a point p coplanar with the triangle t (CGAL's coplanar_side_of_bounded_circle with perturb = true); d is
// a point off the plane that makes (t, d) positive and gives the plane its orientation.  > 0: in conflict.
__device__ int incircle_perturbed(const Pred& P, const int4& fin, int dk, uint32_t p, uint32_t* err)
{
    // fin: the finite cell behind the hull face, dk: the index of its vertex off the face; p is inside the face's circumcircle
    // iff it is inside the circumsphere of fin
    const int s = dt::insphere(P, vget(fin, 0), vget(fin, 1), vget(fin, 2), vget(fin, 3), p);
    if (s) return s;
    int tk[3], m = 0;
    for (int i = 0; i < 4; i++) if (i != dk) tk[m++] = i;
    uint32_t id[4] = {vget(fin, tk[0]), vget(fin, tk[1]), vget(fin, tk[2]), p};
    int pos[4] = {0, 1, 2, 3};
    for (int i = 1; i < 4; i++)
        for (int j = i; j > 0 && dt::lex_less(P, id[pos[j]], id[pos[j - 1]]); j--) { const int t = pos[j]; pos[j] = pos[j - 1]; pos[j - 1] = t; }
    for (int i = 3; i > 0; i--) {
        const int k = pos[i];
        if (k == 3) return -1;
        // the triangle with vertex k replaced by p, against d: its orientation relative to the triangle's own (which is +1 here)
        const int o = orient_rep(P, fin, tk[k], p);
        if (o) return o;
    }
    atomicOr(err, DTE_PERTURB);
    return -1;
}

// conflict of cell c with point p (the Bowyer-Watson test): > 0 yes
__device__ int conflict(const Pred& P, const int4* __restrict__ verts, const uint4* __restrict__ nbr, uint32_t c, uint32_t p, uint32_t* err)
{
    const int4 v = verts[c];
    const int k = inf_index(v);
    if (k < 0) return insphere_perturbed(P, v, p, err);
    const int o = orient_rep(P, v, k, p);
    if (o) return o;
    const uint32_t f = nget(nbr[c], k);
    return incircle_perturbed(P, verts[f >> 2], (int)(f & 3), p, err);
}

// finite cell c contains q (closed)
__device__ bool contains(const Pred& P, const int4& v, uint32_t q)
{
    for (int i = 0; i < 4; i++)
        if (orient_rep(P, v, i, q) < 0) return false;
    return true;
}

// a cell among [base, base + count) for point q: the first finite one that contains it, else the first infinite one it conflicts with
__device__ uint32_t locate_in(const Pred& P, const int4* verts, const uint4* nbr, const uint32_t* kill, uint32_t base, uint32_t count,
                              uint32_t q, uint32_t* err)
{
    for (uint32_t c = base; c < base + count; c++) {
        if (kill && kill[c] != DT_NONE) continue;
        const int4 v = verts[c];
        if (inf_index(v) < 0 && contains(P, v, q)) return c;
    }
    for (uint32_t c = base; c < base + count; c++) {
        if (kill && kill[c] != DT_NONE) continue;
        if (inf_index(verts[c]) >= 0 && conflict(P, verts, nbr, c, q, err) > 0) return c;
    }
    return DT_NONE;
}

// priority of a nominee: a bijection of [0, 2^31) (so priorities are unique and never DT_NONE) that scatters neighbouring Morton
// indices, so that local minima -- winners -- are frequent (with the index itself, only about one nominee per round wins)
__device__ __forceinline__ uint32_t priority(uint32_t q)
{
    q = (q * 0x9E3779B1u) & 0x7FFFFFFFu;
    q ^= q >> 15;
    q = (q * 0x85EBCA77u) & 0x7FFFFFFFu;
    q ^= q >> 13;
    return q;
}

// The nominee of a cell: the first DT_DIRS positions (the extreme points, dt_extremes) before all others, the others in priority order --
// a pseudo-random choice.  (The smallest position would follow the Morton curve: each insertion's neighbour would be nominated next,
// and a region would refine one point per round.)  The point is the low word of the key.
__device__ __forceinline__ unsigned long long nominee_key(uint32_t q)
{
    const uint32_t hi = q < (uint32_t)DT_DIRS ? q : (uint32_t)DT_DIRS + priority(q);
    return ((unsigned long long)hi << 32) | q;
}

__device__ __forceinline__ uint32_t float_key(float f) { return ordered32(f == 0.0f ? 0.0f : f); }     // -0 and +0 are one coordinate

// ---------------------------------------------------------------------------------------------------------------------------
// dedup and Morton order
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DT_THREADS) dt_keys(const float* __restrict__ pts, uint32_t n, int axis, const uint32_t* __restrict__ order,
                                                       uint32_t* __restrict__ key, uint32_t* __restrict__ val, DtHeader* hdr)
{
    const uint32_t i = blockIdx.x * DT_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = order ? order[i] : i;
    const float f = pts[3 * (size_t)j + axis];
    if (!order && !(fabsf(pts[3 * (size_t)i]) <= 3.4028235e38f && fabsf(pts[3 * (size_t)i + 1]) <= 3.4028235e38f &&
                    fabsf(pts[3 * (size_t)i + 2]) <= 3.4028235e38f))
        hdr->nonfinite = 1;
    key[i] = float_key(f);
    val[i] = j;
}

// flag[i] = 1 if sorted point i differs from sorted point i - 1 (the first of a run of duplicates: the lowest input index)
__global__ void __launch_bounds__(DT_THREADS) dt_first_of_run(const float* __restrict__ pts, uint32_t n, const uint32_t* __restrict__ order,
                                                               uint32_t* __restrict__ flag)
{
    const uint32_t i = blockIdx.x * DT_THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t f = 1;
    if (i > 0) {
        const float* a = pts + 3 * (size_t)order[i];
        const float* b = pts + 3 * (size_t)order[i - 1];
        f = !(a[0] == b[0] && a[1] == b[1] && a[2] == b[2]);
    }
    flag[i] = f;
}

__global__ void __launch_bounds__(DT_THREADS) dt_compact_distinct(uint32_t n, const uint32_t* __restrict__ order, const uint32_t* __restrict__ flag,
                                                                   const uint32_t* __restrict__ pos, uint32_t* __restrict__ out, DtHeader* hdr)
{
    const uint32_t i = blockIdx.x * DT_THREADS + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) out[pos[i]] = order[i];
    if (i == n - 1) hdr->ndistinct = pos[i] + flag[i];
}

__global__ void __launch_bounds__(DT_THREADS) dt_bbox(const float* __restrict__ pts, uint32_t m, const uint32_t* __restrict__ ids, DtHeader* hdr)
{
    const uint32_t i = blockIdx.x * DT_THREADS + threadIdx.x;
    if (i >= m) return;
    const float* q = pts + 3 * (size_t)ids[i];
    for (int k = 0; k < 3; k++) {
        const uint32_t key = float_key(q[k]);
        atomicMin(&hdr->bbox[k], key);
        atomicMax(&hdr->bbox[3 + k], key);
    }
}

// The extreme points of the set along DT_DIRS directions (a Fibonacci sphere, in bounding-box units) go first: they are inserted in
// the first rounds, so that the hull soon covers nearly all points.  A point outside the current hull conflicts with every hull
// face it sees, and while the hull is small these cavities overlap and the rounds insert one point each.
__device__ __forceinline__ void dt_dir(int d, double& x, double& y, double& z)
{
    const double zz = 1.0 - (2.0 * d + 1.0) / DT_DIRS;
    const double r = sqrt(1.0 - zz * zz), a = 2.399963229728653 * d;      // golden angle
    x = r * cos(a); y = r * sin(a); z = zz;
}

__global__ void __launch_bounds__(DT_THREADS) dt_extremes(const float* __restrict__ pts, uint32_t m, const uint32_t* __restrict__ ids,
                                                           const DtHeader* __restrict__ hdr, unsigned long long* __restrict__ best)
{
    __shared__ unsigned long long sbest[DT_DIRS];
    for (int d = threadIdx.x; d < DT_DIRS; d += DT_THREADS) sbest[d] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * DT_THREADS + threadIdx.x;
    if (i < m) {
        const float* q = pts + 3 * (size_t)ids[i];
        double t[3];
        for (int k = 0; k < 3; k++) {
            const double lo = unordered32(hdr->bbox[k]), hi = unordered32(hdr->bbox[3 + k]);
            t[k] = hi > lo ? ((double)q[k] - lo) / (hi - lo) : 0.0;
        }
        for (int d = 0; d < DT_DIRS; d++) {
            double x, y, z;
            dt_dir(d, x, y, z);
            const float dot = (float)(x * (t[0] - 0.5) + y * (t[1] - 0.5) + z * (t[2] - 0.5));
            // largest dot first, then the smallest position (unique: the position is in the low word)
            const unsigned long long key = ((unsigned long long)float_key(dot) << 32) | (unsigned long long)(0xFFFFFFFFu - i);
            atomicMax(&sbest[d], key);
        }
    }
    __syncthreads();
    for (int d = threadIdx.x; d < DT_DIRS; d += DT_THREADS)
        if (sbest[d]) atomicMax(&best[d], sbest[d]);
}

__global__ void dt_mark_extremes(const unsigned long long* __restrict__ best, uint32_t* __restrict__ flag)
{
    for (int d = threadIdx.x; d < DT_DIRS; d += blockDim.x) flag[0xFFFFFFFFu - (uint32_t)(best[d] & 0xFFFFFFFFull)] = 1;
}

__global__ void __launch_bounds__(DT_THREADS) dt_morton(const float* __restrict__ pts, uint32_t m, const uint32_t* __restrict__ ids,
                                                         const DtHeader* __restrict__ hdr, const uint32_t* __restrict__ extreme,
                                                         uint32_t* __restrict__ key, uint32_t* __restrict__ val)
{
    const uint32_t i = blockIdx.x * DT_THREADS + threadIdx.x;
    if (i >= m) return;
    const float* q = pts + 3 * (size_t)ids[i];
    uint32_t code = 0;
    for (int k = 0; k < 3; k++) {
        const double lo = unordered32(hdr->bbox[k]), hi = unordered32(hdr->bbox[3 + k]);
        const double ext = hi - lo;
        double t = ext > 0 ? ((double)q[k] - lo) / ext * 1023.0 : 0.0;
        const uint32_t c = t <= 0 ? 0u : t >= 1023.0 ? 1023u : (uint32_t)t;
        code |= morton_spread10(c & 0x3FF) << k;
    }
    key[i] = extreme[i] ? 0u : code + 1;
    val[i] = ids[i];
}

__global__ void __launch_bounds__(DT_THREADS) dt_gather_points(const float* __restrict__ pts, uint32_t m, const uint32_t* __restrict__ ids,
                                                                float* __restrict__ xyz, uint32_t* __restrict__ orig, uint32_t* __restrict__ pt_cell)
{
    const uint32_t i = blockIdx.x * DT_THREADS + threadIdx.x;
    if (i >= m) return;
    const uint32_t j = ids[i];
    for (int k = 0; k < 3; k++) xyz[3 * (size_t)i + k] = pts[3 * (size_t)j + k];
    orig[i] = j;
    pt_cell[i] = 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// start: 4 affinely independent points, 1 finite + 4 infinite cells
// ---------------------------------------------------------------------------------------------------------------------------
// exact test: p0, p1, q collinear ((p1 - p0) x (q - p0) == 0)
__device__ __attribute__((noinline)) bool collinear_exact(const Pred& P, uint32_t a, uint32_t b, uint32_t q)
{
    atomicAdd(P.exact_count, 1ull);
    const float* pa = P.xyz + 3 * (size_t)a;
    const float* pb = P.xyz + 3 * (size_t)b;
    const float* pq = P.xyz + 3 * (size_t)q;
    double u[3][2], v[3][2];
    int un[3], vn[3];
    for (int k = 0; k < 3; k++) { un[k] = dt::x_diff(pb[k], pa[k], u[k]); vn[k] = dt::x_diff(pq[k], pa[k], v[k]); }
    double c[dt::XN], t1[dt::XN], t2[dt::XN];
    for (int k = 0; k < 3; k++) {
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        int nc;
        if (!dt::x_minor(un[i], u[i], vn[j], v[j], un[j], u[j], vn[i], v[i], nc, c, t1, t2)) { atomicOr(P.err, DTE_EXPANSION); return true; }
        if (dt::x_sign(nc, c) != 0) return false;
    }
    return true;
}

// the same with an fp64 filter first: a component of the cross product that is clearly non-zero decides (error of a component
// < 6 eps of its permanent: two rounded differences per product, the product, the subtraction)
__device__ bool collinear(const Pred& P, uint32_t a, uint32_t b, uint32_t q)
{
    const float* pa = P.xyz + 3 * (size_t)a;
    const float* pb = P.xyz + 3 * (size_t)b;
    const float* pq = P.xyz + 3 * (size_t)q;
    double u[3], v[3];
    for (int k = 0; k < 3; k++) { u[k] = (double)pb[k] - pa[k]; v[k] = (double)pq[k] - pa[k]; }
    for (int k = 0; k < 3; k++) {
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        const double p1 = u[i] * v[j], p2 = u[j] * v[i];
        const double perm = fabs(p1) + fabs(p2);
        if (perm > dt::TINY && fabs(p1 - p2) > dt::ORIENT_ERR * perm) return false;
    }
    return collinear_exact(P, a, b, q);
}

__global__ void __launch_bounds__(DT_THREADS) dt_find_start(Pred P, uint32_t m, int which, DtHeader* hdr)
{
    const uint32_t i = blockIdx.x * DT_THREADS + threadIdx.x;
    if (i >= m || i < 2) return;
    const uint32_t* s = hdr->start;
    if (which == 2) {
        if (!collinear(P, s[0], s[1], i)) atomicMin(&hdr->start[2], i);
    } else {
        if (s[2] == DT_NONE || i <= s[2]) return;
        if (dt::orient(P, s[0], s[1], s[2], i) != 0) atomicMin(&hdr->start[3], i);
    }
}

__global__ void dt_init_cells(Pred P, DtHeader* hdr, int4* __restrict__ verts, uint4* __restrict__ nbr, uint32_t* __restrict__ kill,
                              uint32_t* __restrict__ pt_cell)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t a = hdr->start[0], b = hdr->start[1], c = hdr->start[2], d = hdr->start[3];
    if (dt::orient(P, a, b, c, d) < 0) { const uint32_t t = c; c = d; d = t; }
    int4 cell[5];
    cell[0] = make_int4((int)a, (int)b, (int)c, (int)d);
    for (int f = 0; f < 4; f++) {
        int4 v = cell[0];
        vset(v, f, DT_INF);
        const int i = (f + 1) & 3, j = (f + 2) & 3;          // flip the orientation: swap two finite vertices
        const uint32_t t = vget(v, i); vset(v, i, vget(v, j)); vset(v, j, t);
        cell[1 + f] = v;
    }
    for (int x = 0; x < 5; x++) {
        uint4 nb = make_uint4(0, 0, 0, 0);
        for (int f = 0; f < 4; f++) {
            const uint32_t opp = vget(cell[x], f);
            for (int y = 0; y < 5; y++) {
                if (y == x) continue;
                // y shares face f of x if it holds every vertex of x but opp
                int shared = 0, g = -1;
                for (int k = 0; k < 4; k++) {
                    const uint32_t w = vget(cell[y], k);
                    bool in = false;
                    for (int l = 0; l < 4; l++) if (l != f && vget(cell[x], l) == w) in = true;
                    if (in) shared++; else g = k;
                }
                if (shared == 3 && vget(cell[y], g) != opp) nset(nb, f, 4u * y + g);
            }
        }
        verts[x] = cell[x];
        nbr[x] = nb;
        kill[x] = DT_NONE;
    }
    for (int x = 0; x < 4; x++) pt_cell[hdr->start[x]] = PT_DONE;
    hdr->ncells = 5;
}

__global__ void __launch_bounds__(DT_THREADS) dt_locate_initial(Pred P, uint32_t m, const int4* __restrict__ verts, const uint4* __restrict__ nbr,
                                                                 uint32_t* __restrict__ pt_cell)
{
    const uint32_t q = blockIdx.x * DT_THREADS + threadIdx.x;
    if (q >= m || pt_cell[q] == PT_DONE) return;
    const uint32_t c = locate_in(P, verts, nbr, nullptr, 0, 5, q, P.err);
    pt_cell[q] = c == DT_NONE ? PT_LOST : c;
}

// ---------------------------------------------------------------------------------------------------------------------------
// one round
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DT_THREADS) dt_reset(uint32_t ncells, uint32_t* __restrict__ claim, unsigned long long* __restrict__ nominee, DtHeader* hdr)
{
    const uint32_t c = blockIdx.x * DT_THREADS + threadIdx.x;
    if (c == 0) { hdr->winners = 0; hdr->need = 0; hdr->nslots = 0; hdr->bigmin = DT_NONE; hdr->slow_done = 0; hdr->slow_nc = 0; hdr->slow_nf = 0; }
    if (c >= ncells) return;
    claim[c] = DT_NONE;
    nominee[c] = ~0ull;
}

// A finite cell nominates by nominee_key; an infinite cell nominates the point farthest beyond its hull face (fp64 volume, a
// heuristic), as QuickHull does: that point is a vertex of the final hull, and the exterior points -- whose cavities hold every hull
// face they see and overlap each other -- become interior fastest.
__global__ void __launch_bounds__(DT_THREADS) dt_nominate(uint32_t m, const float* __restrict__ xyz, const int4* __restrict__ verts,
                                                           const uint32_t* __restrict__ pt_cell, unsigned long long* __restrict__ nominee)
{
    const uint32_t q = blockIdx.x * DT_THREADS + threadIdx.x;
    if (q >= m) return;
    const uint32_t c = pt_cell[q];
    if (c >= PT_LOST) return;
    const int4 v = verts[c];
    const int k = inf_index(v);
    if (k < 0) { atomicMin(&nominee[c], nominee_key(q)); return; }
    double r[3][3];
    int m3 = 0;
    const float* pq = xyz + 3 * (size_t)q;
    for (int i = 0; i < 4; i++) {
        if (i == k) continue;
        const float* a = xyz + 3 * (size_t)vget(v, i);
        for (int j = 0; j < 3; j++) r[m3][j] = (double)a[j] - pq[j];
        m3++;
    }
    double dist = r[0][0] * (r[1][1] * r[2][2] - r[1][2] * r[2][1]) - r[0][1] * (r[1][0] * r[2][2] - r[1][2] * r[2][0]) +
                  r[0][2] * (r[1][0] * r[2][1] - r[1][1] * r[2][0]);
    dist = fabs(dist);
    const uint32_t hi = ~float_key((float)dist);
    atomicMin(&nominee[c], ((unsigned long long)hi << 32) | q);
}

__global__ void __launch_bounds__(DT_THREADS) dt_gather_slots(uint32_t ncells, const unsigned long long* __restrict__ nominee, uint32_t nslot,
                                                               uint32_t* __restrict__ slots, DtHeader* hdr)
{
    const uint32_t c = blockIdx.x * DT_THREADS + threadIdx.x;
    if (c >= ncells || nominee[c] == ~0ull) return;
    const uint32_t s = atomicAdd(&hdr->nslots, 1u);
    if (s < nslot) {
        uint32_t* sl = slots + (size_t)s * DT_SLOT_WORDS;
        sl[0] = (uint32_t)(nominee[c] & 0xFFFFFFFFull);
        sl[1] = c;
    }
}

// Conflict cavity of p grown from cell `start` by a walk across faces.  Cavity cells go to cav[], boundary faces (4 * cell + face)
// to faces[].  Membership: the cavity list itself (fast path) or mark[c] == p | 2^31 (slow path, which runs alone).  false: overflow.
__device__ bool grow_cavity(const Pred& P, const int4* verts, const uint4* nbr, uint32_t p, uint32_t start, uint32_t* cav, uint32_t maxc,
                            uint32_t* faces, uint32_t maxf, uint32_t* mark, uint32_t& nc, uint32_t& nf)
{
    const uint32_t mv = p | 0x80000000u;      // (never a priority, which is < 2^31)
    nc = 0; nf = 0;
    cav[nc++] = start;
    if (mark) mark[start] = mv;
    for (uint32_t i = 0; i < nc; i++) {
        const uint32_t x = cav[i];
        const uint4 nb = nbr[x];
        for (int j = 0; j < 4; j++) {
            const uint32_t y = nget(nb, j) >> 2;
            bool in = false;
            if (mark) in = mark[y] == mv;
            else for (uint32_t k = 0; k < nc && !in; k++) in = cav[k] == y;
            if (in) continue;
            if (conflict(P, verts, nbr, y, p, P.err) > 0) {
                if (nc >= maxc) return false;
                cav[nc++] = y;
                if (mark) mark[y] = mv;
            } else {
                if (nf >= maxf) return false;
                faces[nf++] = 4 * x + j;
            }
        }
    }
    return true;
}

__global__ void __launch_bounds__(64) dt_grow(Pred P, const int4* __restrict__ verts, const uint4* __restrict__ nbr, uint32_t nslot,
                                              uint32_t* __restrict__ slots, uint32_t* __restrict__ claim, DtHeader* hdr)
{
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    const uint32_t used = hdr->nslots < nslot ? hdr->nslots : nslot;
    if (s >= used) return;
    uint32_t* sl = slots + (size_t)s * DT_SLOT_WORDS;
    const uint32_t p = sl[0];
    uint32_t* cav = sl + 4;
    uint32_t* faces = cav + DT_FAST_CELLS;
    uint32_t nc, nf;
    if (conflict(P, verts, nbr, sl[1], p, P.err) <= 0) { atomicOr(P.err, DTE_LOCATE); sl[2] = 0; return; }
    if (!grow_cavity(P, verts, nbr, p, sl[1], cav, DT_FAST_CELLS, faces, DT_FAST_FACES, nullptr, nc, nf)) {
        sl[2] = 0; sl[3] = 0;
        atomicMin(&hdr->bigmin, p);
        return;
    }
    sl[2] = nc;
    sl[3] = nf;
    const uint32_t pr = priority(p);
    for (uint32_t i = 0; i < nc; i++) atomicMin(&claim[cav[i]], pr);
    for (uint32_t i = 0; i < nf; i++) atomicMin(&claim[nget(nbr[faces[i] >> 2], faces[i] & 3) >> 2], pr);
}

__global__ void __launch_bounds__(64) dt_check(const uint4* __restrict__ nbr, uint32_t nslot, uint32_t* __restrict__ slots,
                                               const uint32_t* __restrict__ claim, DtHeader* hdr)
{
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    const uint32_t used = hdr->nslots < nslot ? hdr->nslots : nslot;
    if (s >= used) return;
    uint32_t* sl = slots + (size_t)s * DT_SLOT_WORDS;
    const uint32_t p = sl[0], nc = sl[2], nf = sl[3];
    if (nc == 0) return;
    const uint32_t* cav = sl + 4;
    const uint32_t* faces = cav + DT_FAST_CELLS;
    const uint32_t pr = priority(p);
    bool win = true;
    for (uint32_t i = 0; i < nc && win; i++) win = claim[cav[i]] == pr;
    for (uint32_t i = 0; i < nf && win; i++) win = claim[nget(nbr[faces[i] >> 2], faces[i] & 3) >> 2] == pr;
    if (!win) { sl[2] = 0; return; }
    atomicAdd(&hdr->winners, 1u);
    atomicAdd(&hdr->need, nf);
}

// Replace the cavity: kill its cells, one new cell per boundary face (the cavity cell with the face's opposite vertex replaced by
// p), linked to the outer cell; the cavity cell's pointer across the face is redirected to the new cell for link_new_cells.
__device__ void commit_cells(const Pred& P, int4* verts, uint4* nbr, uint32_t* kill, unsigned long long* nominee, uint32_t* claim, uint32_t p,
                             const uint32_t* cav, uint32_t nc, const uint32_t* faces, uint32_t nf, uint32_t base, uint32_t* err)
{
    for (uint32_t i = 0; i < nc; i++) kill[cav[i]] = p;
    for (uint32_t t = 0; t < nf; t++) {
        const uint32_t x = faces[t] >> 2;
        const int k = (int)(faces[t] & 3);
        const uint32_t nnew = base + t;
        uint4 xn = nbr[x];
        const uint32_t outer = nget(xn, k);
        int4 v = verts[x];
        vset(v, k, p);
        if (inf_index(v) < 0 && dt::orient(P, vget(v, 0), vget(v, 1), vget(v, 2), vget(v, 3)) <= 0) atomicOr(err, DTE_ORIENT);
        verts[nnew] = v;
        uint4 nn = make_uint4(DT_NONE, DT_NONE, DT_NONE, DT_NONE);
        nset(nn, k, outer);
        nbr[nnew] = nn;
        kill[nnew] = DT_NONE;
        nominee[nnew] = ~0ull;
        claim[nnew] = DT_NONE;
        uint4 on = nbr[outer >> 2];
        nset(on, (int)(outer & 3), 4 * nnew + k);
        nbr[outer >> 2] = on;
        nset(xn, k, 4 * nnew + k);
        nbr[x] = xn;
    }
}

// Link the new cells among themselves: across the face of new cell (x, k) opposite vertex j, rotate about the edge
// verts[x] \ {verts[x][k], verts[x][j]} through the cavity to the other boundary face that holds the edge.
__device__ void link_new_cells(const int4* verts, uint4* nbr, const uint32_t* kill, uint32_t p, const uint32_t* faces, uint32_t nf,
                               uint32_t base, uint32_t* err)
{
    for (uint32_t t = 0; t < nf; t++) {
        const uint32_t x = faces[t] >> 2;
        const int k = (int)(faces[t] & 3);
        const uint32_t nnew = base + t;
        const int4 xv = verts[x];
        uint4 nn = nbr[nnew];
        for (int j = 0; j < 4; j++) {
            if (j == k) continue;
            uint32_t cur = x, s = vget(xv, j), tt = vget(xv, k);
            uint32_t link = DT_NONE;
            for (int step = 0; step < (1 << 20); step++) {
                const int4 cv = verts[cur];
                const int ks = vindex(cv, s);
                const uint32_t y = nget(nbr[cur], ks);
                const uint32_t yc = y >> 2;
                if (kill[yc] != p) { link = 4 * yc + (uint32_t)vindex(cv, tt); break; }
                const uint32_t mv = vget(verts[yc], (int)(y & 3));
                cur = yc; s = tt; tt = mv;
            }
            if (link == DT_NONE) atomicOr(err, DTE_WALK);
            nset(nn, j, link);
        }
        nbr[nnew] = nn;
    }
}

__global__ void __launch_bounds__(64) dt_commit(Pred P, int4* __restrict__ verts, uint4* __restrict__ nbr, uint32_t* __restrict__ kill,
                                                unsigned long long* __restrict__ nominee, uint32_t* __restrict__ claim, uint32_t nslot,
                                                const uint32_t* __restrict__ slots, uint32_t* __restrict__ pt_cell, uint32_t* __restrict__ newbase,
                                                uint32_t* __restrict__ newcount, DtHeader* hdr)
{
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    const uint32_t used = hdr->nslots < nslot ? hdr->nslots : nslot;
    if (s >= used) return;
    const uint32_t* sl = slots + (size_t)s * DT_SLOT_WORDS;
    const uint32_t p = sl[0], nc = sl[2], nf = sl[3];
    if (nc == 0) return;
    const uint32_t base = atomicAdd(&hdr->ncells, nf);
    newbase[p] = base;
    newcount[p] = nf;
    pt_cell[p] = PT_DONE;
    commit_cells(P, verts, nbr, kill, nominee, claim, p, sl + 4, nc, sl + 4 + DT_FAST_CELLS, nf, base, P.err);
}

__global__ void __launch_bounds__(64) dt_link(int4* __restrict__ verts, uint4* __restrict__ nbr, const uint32_t* __restrict__ kill, uint32_t nslot,
                                              const uint32_t* __restrict__ slots, const uint32_t* __restrict__ newbase, DtHeader* hdr)
{
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    const uint32_t used = hdr->nslots < nslot ? hdr->nslots : nslot;
    if (s >= used) return;
    const uint32_t* sl = slots + (size_t)s * DT_SLOT_WORDS;
    const uint32_t p = sl[0], nc = sl[2], nf = sl[3];
    if (nc == 0) return;
    link_new_cells(verts, nbr, kill, p, sl + 4 + DT_FAST_CELLS, nf, newbase[p], &hdr->err);
}

// The slow path: the smallest nominee whose cavity outgrew its slot, grown by one thread with the cavity lists in the inactive cell
// buffers (marks in kill, which no kernel of this phase reads) and claimed like the fast nominees, before dt_check.
__global__ void dt_slow_grow(Pred P, const int4* __restrict__ verts, const uint4* __restrict__ nbr, uint32_t* __restrict__ kill,
                             uint32_t* __restrict__ claim, const uint32_t* __restrict__ pt_cell, uint32_t* __restrict__ cav,
                             uint32_t* __restrict__ faces, uint32_t cap, DtHeader* hdr)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t p = hdr->bigmin;
    if (p == DT_NONE) return;
    uint32_t nc, nf;
    const bool ok = grow_cavity(P, verts, nbr, p, pt_cell[p], cav, cap, faces, cap, kill, nc, nf);
    for (uint32_t i = 0; i < nc; i++) kill[cav[i]] = DT_NONE;
    if (!ok) { atomicOr(&hdr->err, DTE_CAPACITY); return; }
    // priority 0, which no fast nominee has (priority(q) = 0 only for q = 0, a start point): the slow nominee always wins
    for (uint32_t i = 0; i < nc; i++) atomicMin(&claim[cav[i]], 0u);
    for (uint32_t i = 0; i < nf; i++) atomicMin(&claim[nget(nbr[faces[i] >> 2], faces[i] & 3) >> 2], 0u);
    hdr->slow_nc = nc;
    hdr->slow_nf = nf;
}

// after dt_check and the host's capacity check: the slow nominee commits (its claims won)
__global__ void dt_slow_commit(Pred P, int4* __restrict__ verts, uint4* __restrict__ nbr, uint32_t* __restrict__ kill,
                               unsigned long long* __restrict__ nominee, uint32_t* __restrict__ claim, uint32_t* __restrict__ pt_cell,
                               uint32_t* __restrict__ newbase, uint32_t* __restrict__ newcount, const uint32_t* __restrict__ cav,
                               const uint32_t* __restrict__ faces, DtHeader* hdr)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t p = hdr->bigmin, nc = hdr->slow_nc, nf = hdr->slow_nf;
    if (p == DT_NONE || nc == 0) return;
    const uint32_t base = atomicAdd(&hdr->ncells, nf);
    newbase[p] = base;
    newcount[p] = nf;
    pt_cell[p] = PT_DONE;
    commit_cells(P, verts, nbr, kill, nominee, claim, p, cav, nc, faces, nf, base, P.err);
    link_new_cells(verts, nbr, kill, p, faces, nf, base, P.err);
    hdr->slow_done = 1;
}

// points of deleted cells move into the new cells of the point that deleted them
__global__ void __launch_bounds__(DT_THREADS) dt_redistribute(Pred P, uint32_t m, const int4* __restrict__ verts, const uint4* __restrict__ nbr,
                                                               const uint32_t* __restrict__ kill, const uint32_t* __restrict__ newbase,
                                                               const uint32_t* __restrict__ newcount, uint32_t* __restrict__ pt_cell)
{
    const uint32_t q = blockIdx.x * DT_THREADS + threadIdx.x;
    if (q >= m) return;
    const uint32_t c = pt_cell[q];
    if (c >= PT_LOST) return;
    const uint32_t w = kill[c];
    if (w == DT_NONE) return;
    const uint32_t nc = locate_in(P, verts, nbr, nullptr, newbase[w], newcount[w], q, P.err);
    pt_cell[q] = nc == DT_NONE ? PT_LOST : nc;
}

// fallback: a point no new cell took is located by a scan of every live cell
__global__ void __launch_bounds__(DT_THREADS) dt_locate_lost(Pred P, uint32_t m, uint32_t ncells, const int4* __restrict__ verts,
                                                              const uint4* __restrict__ nbr, const uint32_t* __restrict__ kill,
                                                              uint32_t* __restrict__ pt_cell, DtHeader* hdr)
{
    const uint32_t q = blockIdx.x * DT_THREADS + threadIdx.x;
    if (q >= m || pt_cell[q] != PT_LOST) return;
    atomicAdd(&hdr->lost, 1u);
    const uint32_t c = locate_in(P, verts, nbr, kill, 0, ncells, q, P.err);
    if (c == DT_NONE) atomicOr(&hdr->err, DTE_LOCATE);
    pt_cell[q] = c == DT_NONE ? PT_DONE : c;
}

// ---------------------------------------------------------------------------------------------------------------------------
// compaction of the cell arena
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DT_THREADS) dt_live_flags(uint32_t ncells, const uint32_t* __restrict__ kill, uint32_t* __restrict__ flag)
{
    const uint32_t c = blockIdx.x * DT_THREADS + threadIdx.x;
    if (c < ncells) flag[c] = kill[c] == DT_NONE;
}

__global__ void __launch_bounds__(DT_THREADS) dt_scatter_cells(uint32_t ncells, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ map,
                                                                const int4* __restrict__ vin, const uint4* __restrict__ nin, int4* __restrict__ vout,
                                                                uint4* __restrict__ nout)
{
    const uint32_t c = blockIdx.x * DT_THREADS + threadIdx.x;
    if (c >= ncells || !flag[c]) return;
    const uint32_t d = map[c];
    vout[d] = vin[c];
    uint4 nb = nin[c];
    for (int i = 0; i < 4; i++) { const uint32_t x = nget(nb, i); nset(nb, i, 4 * map[x >> 2] + (x & 3)); }
    nout[d] = nb;
}

__global__ void __launch_bounds__(DT_THREADS) dt_remap_points(uint32_t m, const uint32_t* __restrict__ map, uint32_t* __restrict__ pt_cell)
{
    const uint32_t q = blockIdx.x * DT_THREADS + threadIdx.x;
    if (q >= m) return;
    const uint32_t c = pt_cell[q];
    if (c < PT_LOST) pt_cell[q] = map[c];
}

__global__ void __launch_bounds__(DT_THREADS) dt_fill(uint32_t n, uint32_t* __restrict__ a, uint32_t v)
{
    const uint32_t i = blockIdx.x * DT_THREADS + threadIdx.x;
    if (i < n) a[i] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// emit: finite live cells in input indices, canonical, sorted
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DT_THREADS) dt_finite_flags(uint32_t ncells, const int4* __restrict__ verts, const uint32_t* __restrict__ kill,
                                                               uint32_t* __restrict__ flag)
{
    const uint32_t c = blockIdx.x * DT_THREADS + threadIdx.x;
    if (c < ncells) flag[c] = kill[c] == DT_NONE && inf_index(verts[c]) < 0;
}

__global__ void __launch_bounds__(DT_THREADS) dt_canonical(uint32_t ncells, const int4* __restrict__ verts, const uint32_t* __restrict__ flag,
                                                            const uint32_t* __restrict__ map, const uint32_t* __restrict__ orig,
                                                            int4* __restrict__ out, uint32_t* __restrict__ key, uint32_t* __restrict__ val)
{
    const uint32_t c = blockIdx.x * DT_THREADS + threadIdx.x;
    if (c >= ncells || !flag[c]) return;
    const int4 v = verts[c];
    uint32_t a[4];
    for (int i = 0; i < 4; i++) a[i] = orig[vget(v, i)];
    int m = 0;
    for (int i = 1; i < 4; i++) if (a[i] < a[m]) m = i;
    // an even permutation that brings position m to the front: (0123), (1032), (2301), (3210)
    uint32_t b[4];
    for (int i = 0; i < 4; i++) b[i] = a[i ^ m];
    // rotate the last three cyclically so that the smallest of them comes second
    int r = 1;
    for (int i = 2; i < 4; i++) if (b[i] < b[r]) r = i;
    const uint32_t t1 = b[1], t2 = b[2], t3 = b[3];
    if (r == 2) { b[1] = t2; b[2] = t3; b[3] = t1; }
    else if (r == 3) { b[1] = t3; b[2] = t1; b[3] = t2; }
    const uint32_t d = map[c];
    out[d] = make_int4((int)b[0], (int)b[1], (int)b[2], (int)b[3]);
    key[d] = b[3];
    val[d] = d;
}

__global__ void __launch_bounds__(DT_THREADS) dt_sort_key(uint32_t m, const int4* __restrict__ cells, const uint32_t* __restrict__ order, int k,
                                                           uint32_t* __restrict__ key)
{
    const uint32_t i = blockIdx.x * DT_THREADS + threadIdx.x;
    if (i < m) key[i] = vget(cells[order[i]], k);
}

__global__ void __launch_bounds__(DT_THREADS) dt_write_out(uint32_t m, const int4* __restrict__ cells, const uint32_t* __restrict__ order,
                                                            int32_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * DT_THREADS + threadIdx.x;
    if (i >= m) return;
    const int4 v = cells[order[i]];
    out[4 * (size_t)i + 0] = v.x;
    out[4 * (size_t)i + 1] = v.y;
    out[4 * (size_t)i + 2] = v.z;
    out[4 * (size_t)i + 3] = v.w;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------
static int read_header(const DtWs& w, DtHeader* h, hipStream_t st)
{
    GOF_HIP_CHECK(hipMemcpyAsync(h, w.hdr, sizeof(DtHeader), hipMemcpyDeviceToHost, st));
    GOF_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

static int dt_error(const DtHeader& h)
{
    if (h.err & DTE_EXPANSION) set_error("delaunay: an exact predicate outgrew its expansion buffer");
    else if (h.err & DTE_ORIENT) set_error("delaunay: a new cell is not positively oriented");
    else if (h.err & DTE_LOCATE) set_error("delaunay: a point could not be located");
    else if (h.err & DTE_WALK) set_error("delaunay: a cavity edge walk did not close");
    else if (h.err & DTE_PERTURB) set_error("delaunay: the symbolic perturbation did not decide");
    else set_error("delaunay: device error bits 0x%x", h.err);
    return GOF_E_DEVICE;
}

// sort (key, val) pairs in place in w.key[0] / w.val[0] (the result is copied back if it ends in the other buffer)
static int sort_pairs(const DtWs& w, size_t m, int bits, hipStream_t st)
{
    uint32_t *kr, *vr;
    GOF_HIP_CHECK(radix_sort_pairs_u32(w.key[0], w.val[0], w.key[1], w.val[1], m, bits, w.tmp, &kr, &vr, st, nullptr));
    if (kr != w.key[0]) {
        GOF_HIP_CHECK(hipMemcpyAsync(w.key[0], kr, m * 4, hipMemcpyDeviceToDevice, st));
        GOF_HIP_CHECK(hipMemcpyAsync(w.val[0], vr, m * 4, hipMemcpyDeviceToDevice, st));
    }
    return 0;
}

// compacts the live cells into the inactive buffers (and remaps the cells of the npts distinct points); returns the live count
// through *ncells
static int compact(DtWs& w, int& active, uint32_t* ncells, uint32_t npts, hipStream_t st)
{
    const uint32_t nc = *ncells;
    hipLaunchKernelGGL(dt_live_flags, dim3(blocks(nc)), dim3(DT_THREADS), 0, st, nc, w.kill, w.claim);
    const uint32_t* total;
    GOF_HIP_CHECK(device_scan_u32(w.claim, nullptr, w.map, nc, false, w.tmp, &total, st));
    hipLaunchKernelGGL(dt_scatter_cells, dim3(blocks(nc)), dim3(DT_THREADS), 0, st, nc, w.claim, w.map, w.verts[active], w.nbr[active],
                       w.verts[active ^ 1], w.nbr[active ^ 1]);
    hipLaunchKernelGGL(dt_remap_points, dim3(blocks(npts)), dim3(DT_THREADS), 0, st, npts, w.map, w.pt_cell);
    GOF_HIP_CHECK(hipMemcpyAsync(&w.hdr->live, total, 4, hipMemcpyDeviceToDevice, st));
    GOF_HIP_CHECK(hipMemcpyAsync(&w.hdr->ncells, total, 4, hipMemcpyDeviceToDevice, st));
    uint32_t live;
    GOF_HIP_CHECK(hipMemcpyAsync(&live, total, 4, hipMemcpyDeviceToHost, st));
    GOF_HIP_CHECK(hipStreamSynchronize(st));
    hipLaunchKernelGGL(dt_fill, dim3(blocks(nc)), dim3(DT_THREADS), 0, st, nc, w.kill, DT_NONE);
    GOF_HIP_CHECK(hipGetLastError());
    active ^= 1;
    *ncells = live;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// test support: the predicates on caller-chosen index tuples (gof_debug_delaunay_predicates)
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int DT_PROBE_OPS = 7;
constexpr uint32_t DT_PROBE_BAD = 0x80000000u;                 // err[0] while the indices are checked: a query is out of range

__host__ __device__ inline int probe_indices(int op) { return op == 4 ? 3 : (op == 0 || op == 2) ? 4 : 5; }

// flags (in err[0], cleared before) a query whose indices the op would read outside [0, n_points), or whose dk is no vertex slot
__global__ void __launch_bounds__(DT_THREADS) dt_probe_check(uint32_t npts, uint32_t nq, const int32_t* __restrict__ idx, int op,
                                                              uint32_t* __restrict__ err)
{
    const uint32_t q = blockIdx.x * DT_THREADS + threadIdx.x;
    if (q >= nq) return;
    bool bad = false;
    for (int k = 0; k < probe_indices(op); k++) bad |= (uint32_t)idx[6 * (size_t)q + k] >= npts;
    if (op == 6) bad |= (uint32_t)idx[6 * (size_t)q + 5] >= 4u;
    if (bad) atomicOr(&err[0], DT_PROBE_BAD);
}

// one query per thread, with a Pred of its own: the exact evaluations count into the thread's LDS word, the error bits into err[q]
__global__ void __launch_bounds__(DT_THREADS) dt_probe(const float* __restrict__ xyz, uint32_t nq, const int32_t* __restrict__ idx, int op,
                                                        int32_t* __restrict__ sign, uint32_t* __restrict__ exact, uint32_t* __restrict__ err)
{
    __shared__ unsigned long long s_exact[DT_THREADS];
    const uint32_t q = blockIdx.x * DT_THREADS + threadIdx.x;
    if (q >= nq) return;
    s_exact[threadIdx.x] = 0;
    const Pred P = {xyz, &s_exact[threadIdx.x], &err[q]};
    const int32_t* t = idx + 6 * (size_t)q;
    const uint32_t a = (uint32_t)t[0], b = (uint32_t)t[1], c = (uint32_t)t[2], d = (uint32_t)t[3], e = (uint32_t)t[4];
    int s = 0;
    switch (op) {
    case 0: s = dt::orient(P, a, b, c, d); break;
    case 1: s = dt::insphere(P, a, b, c, d, e); break;
    case 2: s = dt::orient_exact(P, a, b, c, d); break;
    case 3: s = dt::insphere_exact(P, a, b, c, d, e); break;
    case 4: s = collinear(P, a, b, c) ? 1 : 0; break;
    case 5: s = insphere_perturbed(P, make_int4((int)a, (int)b, (int)c, (int)d), e, &err[q]); break;
    default: s = incircle_perturbed(P, make_int4((int)a, (int)b, (int)c, (int)d), t[5], e, &err[q]); break;
    }
    sign[q] = s;
    const unsigned long long n = s_exact[threadIdx.x];
    exact[q] = n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n;
}

} // namespace gof

using namespace gof;

extern "C" size_t gof_delaunay_ws_bytes(int64_t n, int64_t tet_capacity)
{
    if (n < 0 || tet_capacity < 0) return 0;
    return dt_layout(n, tet_capacity, nullptr, nullptr) + 256;
}

extern "C" int gof_delaunay_build(int64_t n, const float* points, int64_t tet_capacity, void* ws, size_t ws_bytes, int64_t* num_tets, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!num_tets) { set_error("delaunay: num_tets is NULL"); return GOF_E_INVALID; }
    *num_tets = 0;
    if (n < 0 || n >= ((int64_t)1 << 31)) { set_error("delaunay: n = %lld must be in [0, 2^31)", (long long)n); return GOF_E_INVALID; }
    if (tet_capacity < 16 || tet_capacity > DT_MAX_CELLS - 1) { set_error("delaunay: tet capacity %lld must be in [16, 2^30)", (long long)tet_capacity); return GOF_E_INVALID; }
    if (!ws || ws_bytes < gof_delaunay_ws_bytes(n, tet_capacity)) { set_error("delaunay: workspace too small"); return GOF_E_WORKSPACE; }
    if (n > 0 && !points) { set_error("delaunay: points is NULL"); return GOF_E_INVALID; }
    DtWs w;
    dt_layout(n, tet_capacity, (void*)a256((size_t)ws), &w);
    DtHeader h;
    memset(&h, 0, sizeof(h));
    h.bigmin = DT_NONE;
    for (int k = 0; k < 4; k++) h.start[k] = DT_NONE;
    for (int k = 0; k < 3; k++) { h.bbox[k] = 0xFFFFFFFFu; h.bbox[3 + k] = 0; }
    h.stats[6] = tet_capacity;
    h.n = n;
    h.cap = tet_capacity;
    GOF_HIP_CHECK(hipMemcpyAsync(w.hdr, &h, sizeof(h), hipMemcpyHostToDevice, st));
    const uint32_t N = (uint32_t)n;
    if (N == 0) { GOF_HIP_CHECK(hipStreamSynchronize(st)); return 0; }

    // 1. dedup: three stable passes on the orderable coordinate keys (z, y, x) carrying the input index
    for (int axis = 2; axis >= 0; axis--) {
        hipLaunchKernelGGL(dt_keys, dim3(blocks(N)), dim3(DT_THREADS), 0, st, points, N, axis, axis == 2 ? nullptr : w.val[0], w.key[0],
                           w.val[1], w.hdr);
        // (the gathered indices went to val[1]: move them to val[0] for the sort)
        GOF_HIP_CHECK(hipMemcpyAsync(w.val[0], w.val[1], (size_t)N * 4, hipMemcpyDeviceToDevice, st));
        if (int r = sort_pairs(w, N, 32, st)) return r;
    }
    hipLaunchKernelGGL(dt_first_of_run, dim3(blocks(N)), dim3(DT_THREADS), 0, st, points, N, w.val[0], w.key[1]);
    // (the positions in pt_cell, [n] and free until dt_gather_points)
    GOF_HIP_CHECK(device_scan_u32(w.key[1], nullptr, w.pt_cell, N, false, w.tmp, nullptr, st));
    hipLaunchKernelGGL(dt_compact_distinct, dim3(blocks(N)), dim3(DT_THREADS), 0, st, N, w.val[0], w.key[1], w.pt_cell, w.val[1], w.hdr);
    if (int r = read_header(w, &h, st)) return r;
    if (h.nonfinite) { set_error("delaunay: a point coordinate is not finite"); return GOF_E_INVALID; }
    const uint32_t D = h.ndistinct;
    // 2. Morton order of the distinct points (ties: lexicographic order)
    hipLaunchKernelGGL(dt_bbox, dim3(blocks(D)), dim3(DT_THREADS), 0, st, points, D, w.val[1], w.hdr);
    // (scratch: the extreme flags in key[1], the 26 keys in the sort scratch; both free until the sort)
    unsigned long long* best = reinterpret_cast<unsigned long long*>(w.tmp);
    GOF_HIP_CHECK(hipMemsetAsync(w.key[1], 0, (size_t)D * 4, st));
    GOF_HIP_CHECK(hipMemsetAsync(best, 0, DT_DIRS * 8, st));
    hipLaunchKernelGGL(dt_extremes, dim3(blocks(D)), dim3(DT_THREADS), 0, st, points, D, w.val[1], w.hdr, best);
    hipLaunchKernelGGL(dt_mark_extremes, dim3(1), dim3(64), 0, st, best, w.key[1]);
    hipLaunchKernelGGL(dt_morton, dim3(blocks(D)), dim3(DT_THREADS), 0, st, points, D, w.val[1], w.hdr, w.key[1], w.key[0], w.val[0]);
    if (int r = sort_pairs(w, D, 31, st)) return r;
    hipLaunchKernelGGL(dt_gather_points, dim3(blocks(D)), dim3(DT_THREADS), 0, st, points, D, w.val[0], w.xyz, w.orig, w.pt_cell);
    GOF_HIP_CHECK(hipGetLastError());

    int active = 0;
    Pred P{w.xyz, &w.hdr->exact, &w.hdr->err};
    long long rounds = 0, slow = 0;
    uint32_t ncells = 0, peak = 0;
    if (D >= 4) {
        // 3. start: p0 = 0, p1 = 1, p2 = the first point off their line, p3 = the first point off their plane
        GOF_HIP_CHECK(hipMemsetAsync(w.hdr->start, 0, 4, st));
        const uint32_t one = 1;
        GOF_HIP_CHECK(hipMemcpyAsync(&w.hdr->start[1], &one, 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(dt_find_start, dim3(blocks(D)), dim3(DT_THREADS), 0, st, P, D, 2, w.hdr);
        hipLaunchKernelGGL(dt_find_start, dim3(blocks(D)), dim3(DT_THREADS), 0, st, P, D, 3, w.hdr);
        if (int r = read_header(w, &h, st)) return r;
        if (h.err) return dt_error(h);
    }
    if (D >= 4 && h.start[3] != DT_NONE) {
        hipLaunchKernelGGL(dt_init_cells, dim3(1), dim3(64), 0, st, P, w.hdr, w.verts[0], w.nbr[0], w.kill, w.pt_cell);
        hipLaunchKernelGGL(dt_locate_initial, dim3(blocks(D)), dim3(DT_THREADS), 0, st, P, D, w.verts[0], w.nbr[0], w.pt_cell);
        ncells = 5;
        peak = 5;
        int64_t remaining = (int64_t)D - 4;
        bool compacted = false;
        uint32_t last_live = ncells;
        while (remaining > 0) {
            if (++rounds > DT_MAX_ROUNDS) { set_error("delaunay: no convergence after %d rounds", DT_MAX_ROUNDS); return GOF_E_DEVICE; }
            // compact when the arena is 3/4 full and enough cells were created (and as many killed) since the last compaction
            if (!compacted && (uint64_t)ncells * 4 > (uint64_t)w.cap * 3 && (uint64_t)(ncells - last_live) * 16 > (uint64_t)w.cap) {
                if (int r = compact(w, active, &ncells, D, st)) return r;
                compacted = true;
                last_live = ncells;
            }
            int4* V = w.verts[active];
            uint4* NB = w.nbr[active];
            hipLaunchKernelGGL(dt_reset, dim3(blocks(ncells)), dim3(DT_THREADS), 0, st, ncells, w.claim, w.nominee, w.hdr);
            hipLaunchKernelGGL(dt_nominate, dim3(blocks(D)), dim3(DT_THREADS), 0, st, D, w.xyz, V, w.pt_cell, w.nominee);
            hipLaunchKernelGGL(dt_gather_slots, dim3(blocks(ncells)), dim3(DT_THREADS), 0, st, ncells, w.nominee, (uint32_t)w.nslot, w.slots, w.hdr);
            const uint32_t sb = (uint32_t)((w.nslot + 63) / 64);
            hipLaunchKernelGGL(dt_grow, dim3(sb), dim3(64), 0, st, P, V, NB, (uint32_t)w.nslot, w.slots, w.claim, w.hdr);
            uint32_t* scav = (uint32_t*)w.verts[active ^ 1];
            uint32_t* sfaces = (uint32_t*)w.nbr[active ^ 1];
            hipLaunchKernelGGL(dt_slow_grow, dim3(1), dim3(64), 0, st, P, V, NB, w.kill, w.claim, w.pt_cell, scav, sfaces, (uint32_t)w.cap, w.hdr);
            hipLaunchKernelGGL(dt_check, dim3(sb), dim3(64), 0, st, NB, (uint32_t)w.nslot, w.slots, w.claim, w.hdr);
            if (int r = read_header(w, &h, st)) return r;
            if (h.err & ~DTE_CAPACITY) return dt_error(h);
            const uint64_t need = (uint64_t)h.need + h.slow_nf;
            if ((h.err & DTE_CAPACITY) || (uint64_t)ncells + need > (uint64_t)w.cap) {
                if (!compacted) {
                    GOF_HIP_CHECK(hipMemsetAsync(&w.hdr->err, 0, 4, st));
                    if (int r = compact(w, active, &ncells, D, st)) return r;
                    compacted = true; last_live = ncells; rounds--; continue;
                }
                *num_tets = std::max<int64_t>(w.cap + w.cap / 4, ((int64_t)ncells + (int64_t)need) * 5 / 4);
                if (*num_tets >= DT_MAX_CELLS) *num_tets = DT_MAX_CELLS - 1;
                set_error("delaunay: the cell arena (%lld cells) is too small", (long long)w.cap);
                return GOF_E_CAPACITY;
            }
            if (h.winners == 0 && h.slow_nc == 0) {
                set_error("delaunay: a round without an insertion (%lld points left)", (long long)remaining);
                return GOF_E_DEVICE;
            }
            hipLaunchKernelGGL(dt_slow_commit, dim3(1), dim3(64), 0, st, P, V, NB, w.kill, w.nominee, w.claim, w.pt_cell, w.newbase, w.newcount,
                               scav, sfaces, w.hdr);
            hipLaunchKernelGGL(dt_commit, dim3(sb), dim3(64), 0, st, P, V, NB, w.kill, w.nominee, w.claim, (uint32_t)w.nslot, w.slots, w.pt_cell,
                               w.newbase, w.newcount, w.hdr);
            hipLaunchKernelGGL(dt_link, dim3(sb), dim3(64), 0, st, V, NB, w.kill, (uint32_t)w.nslot, w.slots, w.newbase, w.hdr);
            // (the slow nominee claimed with priority 0: it always wins)
            ncells += (uint32_t)need;
            remaining -= h.winners;
            if (h.slow_nc) { remaining -= 1; slow++; }
            compacted = false;
            if (ncells > peak) peak = ncells;
            hipLaunchKernelGGL(dt_redistribute, dim3(blocks(D)), dim3(DT_THREADS), 0, st, P, D, V, NB, w.kill, w.newbase, w.newcount, w.pt_cell);
            hipLaunchKernelGGL(dt_locate_lost, dim3(blocks(D)), dim3(DT_THREADS), 0, st, P, D, ncells, V, NB, w.kill, w.pt_cell, w.hdr);
            GOF_HIP_CHECK(hipGetLastError());
        }
        // final: drop the dead cells and count the finite ones
        if (int r = compact(w, active, &ncells, D, st)) return r;
        hipLaunchKernelGGL(dt_finite_flags, dim3(blocks(ncells)), dim3(DT_THREADS), 0, st, ncells, w.verts[active], w.kill, w.claim);
        const uint32_t* total;
        GOF_HIP_CHECK(device_scan_u32(w.claim, nullptr, w.map, ncells, false, w.tmp, &total, st));
        GOF_HIP_CHECK(hipMemcpyAsync(&w.hdr->live, total, 4, hipMemcpyDeviceToDevice, st));
        if (int r = read_header(w, &h, st)) return r;
        if (h.err) return dt_error(h);
    } else {
        h.live = 0;
        ncells = 0;
    }
    h.active = (uint32_t)active;
    h.ncells = ncells;
    h.stats[0] = rounds;
    h.stats[1] = (long long)h.exact;
    h.stats[2] = peak;
    h.stats[3] = slow;
    h.stats[4] = h.lost;
    h.stats[5] = D;
    h.stats[6] = tet_capacity;
    h.stats[7] = ncells;
    GOF_HIP_CHECK(hipMemcpyAsync(w.hdr, &h, sizeof(h), hipMemcpyHostToDevice, st));
    GOF_HIP_CHECK(hipStreamSynchronize(st));
    *num_tets = h.live;
    return 0;
}

// the header of a built workspace, and its layout
static int built_layout(const void* ws, DtWs* w, DtHeader* h, hipStream_t st)
{
    if (!ws) { set_error("delaunay: workspace is NULL"); return GOF_E_INVALID; }
    DtWs hw;
    hw.hdr = (DtHeader*)a256((size_t)ws);
    if (int r = read_header(hw, h, st)) return r;
    if (h->n < 0 || h->cap < 16 || h->cap >= DT_MAX_CELLS) { set_error("delaunay: the workspace holds no build"); return GOF_E_INVALID; }
    dt_layout(h->n, h->cap, hw.hdr, w);
    return 0;
}

extern "C" int gof_delaunay_emit(void* ws, int64_t num_tets, int32_t* tets_out, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (num_tets < 0 || (num_tets > 0 && !tets_out)) { set_error("delaunay: bad output"); return GOF_E_INVALID; }
    DtWs w;
    DtHeader h;
    if (int r = built_layout(ws, &w, &h, st)) return r;
    const int64_t n = h.n;
    if ((int64_t)h.live != num_tets) { set_error("delaunay: num_tets %lld does not match the build (%u)", (long long)num_tets, h.live); return GOF_E_INVALID; }
    if (num_tets == 0) return 0;
    const int active = (int)h.active;
    const uint32_t nc = h.ncells, M = (uint32_t)num_tets;
    int4* cells = w.verts[active ^ 1];
    // the sort buffers: the inactive neighbour buffer (4 words per cell of capacity, num_tets <= capacity)
    uint32_t* eb = reinterpret_cast<uint32_t*>(w.nbr[active ^ 1]);
    w.key[0] = eb; w.val[0] = eb + w.cap; w.key[1] = eb + 2 * w.cap; w.val[1] = eb + 3 * w.cap;
    // (dt_finite_flags / map of the build still hold: flags in claim, exclusive positions in map)
    hipLaunchKernelGGL(dt_canonical, dim3(blocks(nc)), dim3(DT_THREADS), 0, st, nc, w.verts[active], w.claim, w.map, w.orig, cells, w.key[0], w.val[0]);
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < n) bits++;
    if (int r = sort_pairs(w, M, bits, st)) return r;
    for (int k = 2; k >= 0; k--) {
        hipLaunchKernelGGL(dt_sort_key, dim3(blocks(M)), dim3(DT_THREADS), 0, st, M, cells, w.val[0], k, w.key[0]);
        if (int r = sort_pairs(w, M, bits, st)) return r;
    }
    hipLaunchKernelGGL(dt_write_out, dim3(blocks(M)), dim3(DT_THREADS), 0, st, M, cells, w.val[0], tets_out);
    GOF_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int gof_delaunay_stats(const void* ws, int64_t* stats, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!stats) { set_error("delaunay: stats is NULL"); return GOF_E_INVALID; }
    DtWs w;
    DtHeader h;
    if (int r = built_layout(ws, &w, &h, st)) return r;
    for (int k = 0; k < 8; k++) stats[k] = h.stats[k];
    return 0;
}

// Test support (include/gof_delaunay_hip.h): the build's own predicate functions on index tuples the caller chooses.
extern "C" int gof_debug_delaunay_predicates(int64_t n_points, const float* xyz, int64_t n_queries, const int32_t* idx, int op, int32_t* sign,
                                             uint32_t* exact, uint32_t* err, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (op < 0 || op >= DT_PROBE_OPS) { set_error("delaunay probe: unknown op %d", op); return GOF_E_INVALID; }
    if (n_points < 0 || n_points >= ((int64_t)1 << 31) || n_queries < 0 || n_queries >= ((int64_t)1 << 31)) {
        set_error("delaunay probe: n_points = %lld, n_queries = %lld must be in [0, 2^31)", (long long)n_points, (long long)n_queries);
        return GOF_E_INVALID;
    }
    if (n_queries == 0) return 0;
    if (!xyz || !idx || !sign || !exact || !err) { set_error("delaunay probe: a pointer is NULL"); return GOF_E_INVALID; }
    const uint32_t nq = (uint32_t)n_queries;
    hipLaunchKernelGGL(dt_fill, dim3(blocks(nq)), dim3(DT_THREADS), 0, st, nq, err, 0u);
    hipLaunchKernelGGL(dt_probe_check, dim3(blocks(nq)), dim3(DT_THREADS), 0, st, (uint32_t)n_points, nq, idx, op, err);
    uint32_t flag = 0;
    GOF_HIP_CHECK(hipMemcpyAsync(&flag, err, 4, hipMemcpyDeviceToHost, st));
    GOF_HIP_CHECK(hipStreamSynchronize(st));
    if (flag & DT_PROBE_BAD) {
        hipLaunchKernelGGL(dt_fill, dim3(1), dim3(DT_THREADS), 0, st, 1u, err, 0u);
        GOF_HIP_CHECK(hipGetLastError());
        set_error("delaunay probe: a query of op %d holds an index outside [0, %lld) (or a vertex slot outside [0, 4))", op, (long long)n_points);
        return GOF_E_INVALID;
    }
    hipLaunchKernelGGL(dt_probe, dim3(blocks(nq)), dim3(DT_THREADS), 0, st, xyz, nq, idx, op, sign, exact, err);
    GOF_HIP_CHECK(hipGetLastError());
    return 0;
}
