// delaunay_predicates.h -- exact orientation and in-sphere tests on float32 points (csrc/delaunay.hip).
//
// Every test first evaluates its determinant in fp64 with a semi-static error bound (Shewchuk-style: |det| > C * eps * permanent,
// C widened for the rounding of the fp64 coordinate differences).  When the bound cannot decide, the determinant is evaluated exactly
// with floating-point expansions (two-sum, two-product through fma): a float32 coordinate difference is a two-term expansion, so no
// exponent gap between inputs loses a bit.  The exact paths are noinline and count themselves into a device counter.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gof {
namespace dt {

constexpr int XN = 128;                      // expansion capacity of the exact paths (tests/test_delaunay_predicates_*: never outgrown)
constexpr double ORIENT_ERR = 2.0e-15;       // ~18 eps (Shewchuk o3derrboundA = 7 eps, + 3 eps for the rounded differences)
constexpr double INSPHERE_ERR = 5.0e-15;     // ~45 eps (isperrboundA = 16 eps, + 5 eps for the rounded differences)
constexpr double TINY = 1e-250;              // below it the fp64 filter could lose bits to underflow: always exact

struct Pred {
    const float* xyz;                        // [n][3]
    unsigned long long* exact_count;         // exact evaluations (statistics)
    uint32_t* err;                           // error word: bit 0 = an expansion outgrew XN
};

__device__ __forceinline__ void two_sum(double a, double b, double& x, double& y)
{
    x = a + b;
    const double bv = x - a, av = x - bv;
    y = (a - av) + (b - bv);
}
__device__ __forceinline__ void fast_two_sum(double a, double b, double& x, double& y)
{
    x = a + b;
    y = b - (x - a);
}
__device__ __forceinline__ void two_prod(double a, double b, double& x, double& y)
{
    x = a * b;
    y = fma(a, b, -x);
}

// e (length n, capacity n + 1) += b, zero-eliminating; returns the new length
__device__ inline int x_grow(int n, double* e, double b)
{
    double q = b;
    int h = 0;
    for (int i = 0; i < n; i++) {
        double qn, hh;
        two_sum(q, e[i], qn, hh);
        q = qn;
        if (hh != 0.0) e[h++] = hh;
    }
    if (q != 0.0 || h == 0) e[h++] = q;
    return h;
}
// in place; the result is non-adjacent with its largest component last
__device__ inline int x_compress(int n, double* e)
{
    if (n <= 1) return n;
    int bottom = n - 1;
    double q = e[bottom];
    for (int i = n - 2; i >= 0; i--) {
        double qn, qq;
        fast_two_sum(q, e[i], qn, qq);
        if (qq != 0.0) { e[bottom--] = qn; q = qq; }
        else q = qn;
    }
    int top = 0;
    for (int i = bottom + 1; i < n; i++) {
        double qn, qq;
        fast_two_sum(e[i], q, qn, qq);
        if (qq != 0.0) e[top++] = qq;
        q = qn;
    }
    e[top++] = q;
    return top;
}
// h = e * b (h holds up to 2n)
__device__ inline int x_scale(int n, const double* e, double b, double* h)
{
    double q, hh;
    two_prod(e[0], b, q, hh);
    int k = 0;
    if (hh != 0.0) h[k++] = hh;
    for (int i = 1; i < n; i++) {
        double p1, p0, s;
        two_prod(e[i], b, p1, p0);
        two_sum(q, p0, s, hh);
        if (hh != 0.0) h[k++] = hh;
        two_sum(p1, s, q, hh);
        if (hh != 0.0) h[k++] = hh;
    }
    if (q != 0.0 || k == 0) h[k++] = q;
    return k;
}
// e (length n) += f (length m), compressed; false if XN would be exceeded
__device__ inline bool x_add(int& n, double* e, int m, const double* f)
{
    if (n + m > XN) return false;
    for (int i = 0; i < m; i++) n = x_grow(n, e, f[i]);
    n = x_compress(n, e);
    return true;
}
// out = a * b; tmp: XN scratch
__device__ inline bool x_mul(int an, const double* a, int bn, const double* b, int& on, double* out, double* tmp)
{
    on = 1;
    out[0] = 0.0;
    if (2 * an > XN) return false;
    for (int j = 0; j < bn; j++) {
        const int t = x_scale(an, a, b[j], tmp);
        if (!x_add(on, out, t, tmp)) return false;
    }
    return true;
}
__device__ inline void x_neg(int n, double* e) { for (int i = 0; i < n; i++) e[i] = -e[i]; }
__device__ inline int x_sign(int n, const double* e) { const double v = e[n - 1]; return (v > 0.0) - (v < 0.0); }
// b - a of two float32 values as an exact expansion of at most two terms
__device__ inline int x_diff(float b, float a, double* e)
{
    double x, y;
    two_sum((double)b, -(double)a, x, y);
    int n = 0;
    if (y != 0.0) e[n++] = y;
    e[n++] = x;
    return n;
}
// c = a0 * b1 - a1 * b0 (2x2 minor of expansions); tmp, tmp2: XN scratch
__device__ inline bool x_minor(int na0, const double* a0, int nb1, const double* b1, int na1, const double* a1, int nb0, const double* b0,
                               int& nc, double* c, double* tmp, double* tmp2)
{
    int n2;
    if (!x_mul(na0, a0, nb1, b1, nc, c, tmp)) return false;
    if (!x_mul(na1, a1, nb0, b0, n2, tmp2, tmp)) return false;
    x_neg(n2, tmp2);
    return x_add(nc, c, n2, tmp2);
}
// det[u; v; w] of 3x3 expansions given as [row][col] arrays of length <= 2 (two-term differences); result in out
__device__ inline bool x_det3(const double (*r)[3][2], const int (*rn)[3], int i0, int i1, int i2, int& on, double* out, double* t0, double* t1,
                              double* t2, double* t3)
{
    // cofactors along row i0: c_x = v_y w_z - v_z w_y, c_y = v_z w_x - v_x w_z, c_z = v_x w_y - v_y w_x
    on = 1;
    out[0] = 0.0;
    for (int k = 0; k < 3; k++) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        int nc, np;
        if (!x_minor(rn[i1][a], r[i1][a], rn[i2][b], r[i2][b], rn[i1][b], r[i1][b], rn[i2][a], r[i2][a], nc, t0, t1, t2)) return false;
        if (!x_mul(rn[i0][k], r[i0][k], nc, t0, np, t3, t1)) return false;
        if (!x_add(on, out, np, t3)) return false;
    }
    return true;
}

__device__ __attribute__((noinline)) int orient_exact(const Pred& P, uint32_t ia, uint32_t ib, uint32_t ic, uint32_t id)
{
    atomicAdd(P.exact_count, 1ull);
    const float* a = P.xyz + 3 * (size_t)ia;
    const uint32_t ids[3] = {ib, ic, id};
    double r[3][3][2];
    int rn[3][3];
    for (int i = 0; i < 3; i++) {
        const float* q = P.xyz + 3 * (size_t)ids[i];
        for (int k = 0; k < 3; k++) rn[i][k] = x_diff(q[k], a[k], r[i][k]);
    }
    double out[XN], t0[XN], t1[XN], t2[XN], t3[XN];
    int on;
    if (!x_det3(r, rn, 0, 1, 2, on, out, t0, t1, t2, t3)) { atomicOr(P.err, 1u); return 0; }
    return x_sign(on, out);
}

__device__ __attribute__((noinline)) int insphere_exact(const Pred& P, uint32_t ia, uint32_t ib, uint32_t ic, uint32_t id, uint32_t ie)
{
    atomicAdd(P.exact_count, 1ull);
    const float* e = P.xyz + 3 * (size_t)ie;
    const uint32_t ids[4] = {ia, ib, ic, id};
    double r[4][3][2];
    int rn[4][3];
    for (int i = 0; i < 4; i++) {
        const float* q = P.xyz + 3 * (size_t)ids[i];
        for (int k = 0; k < 3; k++) rn[i][k] = x_diff(q[k], e[k], r[i][k]);
    }
    double acc[XN], lift[XN], det[XN], t0[XN], t1[XN], t2[XN], t3[XN];
    int nacc = 1;
    acc[0] = 0.0;
    // D = l_a det(b,c,d) - l_b det(a,c,d) + l_c det(a,b,d) - l_d det(a,b,c)   (> 0: e inside the sphere of positive (a,b,c,d))
    const int MINOR[4][3] = {{1, 2, 3}, {0, 2, 3}, {0, 1, 3}, {0, 1, 2}};
    for (int i = 0; i < 4; i++) {
        int nl = 1, nd, np, ns;
        lift[0] = 0.0;
        for (int k = 0; k < 3; k++) {
            if (!x_mul(rn[i][k], r[i][k], rn[i][k], r[i][k], ns, t0, t1)) goto overflow;
            if (!x_add(nl, lift, ns, t0)) goto overflow;
        }
        if (!x_det3(r, rn, MINOR[i][0], MINOR[i][1], MINOR[i][2], nd, det, t0, t1, t2, t3)) goto overflow;
        if (!x_mul(nl, lift, nd, det, np, t0, t1)) goto overflow;
        if (i & 1) x_neg(np, t0);
        if (!x_add(nacc, acc, np, t0)) goto overflow;
    }
    return x_sign(nacc, acc);
overflow:
    atomicOr(P.err, 1u);
    return 0;
}

// sign det[b - a, c - a, d - a]
__device__ inline int orient(const Pred& P, uint32_t ia, uint32_t ib, uint32_t ic, uint32_t id)
{
    const float* a = P.xyz + 3 * (size_t)ia;
    const float* b = P.xyz + 3 * (size_t)ib;
    const float* c = P.xyz + 3 * (size_t)ic;
    const float* d = P.xyz + 3 * (size_t)id;
    const double ax = a[0], ay = a[1], az = a[2];
    const double ux = b[0] - ax, uy = b[1] - ay, uz = b[2] - az;
    const double vx = c[0] - ax, vy = c[1] - ay, vz = c[2] - az;
    const double wx = d[0] - ax, wy = d[1] - ay, wz = d[2] - az;
    const double p1 = vy * wz, p2 = vz * wy, p3 = vz * wx, p4 = vx * wz, p5 = vx * wy, p6 = vy * wx;
    const double det = ux * (p1 - p2) + uy * (p3 - p4) + uz * (p5 - p6);
    const double perm = fabs(ux) * (fabs(p1) + fabs(p2)) + fabs(uy) * (fabs(p3) + fabs(p4)) + fabs(uz) * (fabs(p5) + fabs(p6));
    const double bound = ORIENT_ERR * perm;
    if (perm > TINY) {
        if (det > bound) return 1;
        if (-det > bound) return -1;
    }
    return orient_exact(P, ia, ib, ic, id);
}

__device__ __forceinline__ double det3d(double ux, double uy, double uz, double vx, double vy, double vz, double wx, double wy, double wz,
                                        double& perm)
{
    const double p1 = vy * wz, p2 = vz * wy, p3 = vz * wx, p4 = vx * wz, p5 = vx * wy, p6 = vy * wx;
    perm = fabs(ux) * (fabs(p1) + fabs(p2)) + fabs(uy) * (fabs(p3) + fabs(p4)) + fabs(uz) * (fabs(p5) + fabs(p6));
    return ux * (p1 - p2) + uy * (p3 - p4) + uz * (p5 - p6);
}

// > 0: e strictly inside the circumsphere of the positively oriented (a,b,c,d); 0: on it (not perturbed)
__device__ inline int insphere(const Pred& P, uint32_t ia, uint32_t ib, uint32_t ic, uint32_t id, uint32_t ie)
{
    const uint32_t ids[4] = {ia, ib, ic, id};
    const float* e = P.xyz + 3 * (size_t)ie;
    double x[4], y[4], z[4], l[4];
    for (int i = 0; i < 4; i++) {
        const float* q = P.xyz + 3 * (size_t)ids[i];
        x[i] = (double)q[0] - e[0];
        y[i] = (double)q[1] - e[1];
        z[i] = (double)q[2] - e[2];
        l[i] = x[i] * x[i] + y[i] * y[i] + z[i] * z[i];
    }
    double pa, pb, pc, pd;
    const double da = det3d(x[1], y[1], z[1], x[2], y[2], z[2], x[3], y[3], z[3], pa);
    const double db = det3d(x[0], y[0], z[0], x[2], y[2], z[2], x[3], y[3], z[3], pb);
    const double dc = det3d(x[0], y[0], z[0], x[1], y[1], z[1], x[3], y[3], z[3], pc);
    const double dd = det3d(x[0], y[0], z[0], x[1], y[1], z[1], x[2], y[2], z[2], pd);
    const double det = (l[0] * da - l[1] * db) + (l[2] * dc - l[3] * dd);
    const double perm = (l[0] * pa + l[1] * pb) + (l[2] * pc + l[3] * pd);
    const double bound = INSPHERE_ERR * perm;
    if (perm > TINY) {
        if (det > bound) return 1;
        if (-det > bound) return -1;
    }
    return insphere_exact(P, ia, ib, ic, id, ie);
}

// lexicographic (x, y, z) order of two distinct points: true if a < b
__device__ __forceinline__ bool lex_less(const Pred& P, uint32_t ia, uint32_t ib)
{
    const float* a = P.xyz + 3 * (size_t)ia;
    const float* b = P.xyz + 3 * (size_t)ib;
    if (a[0] != b[0]) return a[0] < b[0];
    if (a[1] != b[1]) return a[1] < b[1];
    return a[2] < b[2];
}

} // namespace dt
} // namespace gof
