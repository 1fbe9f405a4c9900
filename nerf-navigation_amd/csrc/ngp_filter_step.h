// ngp_filter_step.h -- the float64 arithmetic of the pose filter's time step (DESIGN.md §3.5 "Native time step"): forward-mode numbers of first
// order (value, one tangent) and second order (value, two tangents, the mixed term), the reference's rotation formulas written over them, and
// Agent.drone_dynamics (nav/agent_helpers.py:124-171).  Everything is evaluated as the reference writes it -- the `1e-10 + angle` guard with its
// dependence on the angle, the linearised acos, the `theta == 0` and `angle == 0` branches -- under torch autograd's conventions: the norm has a zero
// subgradient at 0, sign() carries no derivative, a masked assignment cuts the derivative.  Plain C++, usable on the host and on the device.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define NFS_HD __host__ __device__ __forceinline__
#else
#define NFS_HD inline
#endif

struct nfs_d1 {                                                              // value and one tangent
    double v, d;
    NFS_HD nfs_d1() : v(0.0), d(0.0) {}
    NFS_HD nfs_d1(double c) : v(c), d(0.0) {}
    NFS_HD nfs_d1(double v_, double d_) : v(v_), d(d_) {}
};
struct nfs_d2 {                                                              // value, the tangents along two directions, the mixed second derivative
    double v, a, b, ab;
    NFS_HD nfs_d2() : v(0.0), a(0.0), b(0.0), ab(0.0) {}
    NFS_HD nfs_d2(double c) : v(c), a(0.0), b(0.0), ab(0.0) {}
    NFS_HD nfs_d2(double v_, double a_, double b_, double ab_) : v(v_), a(a_), b(b_), ab(ab_) {}
};

NFS_HD nfs_d1 operator+(nfs_d1 x, nfs_d1 y) { return {x.v + y.v, x.d + y.d}; }
NFS_HD nfs_d1 operator-(nfs_d1 x, nfs_d1 y) { return {x.v - y.v, x.d - y.d}; }
NFS_HD nfs_d1 operator-(nfs_d1 x) { return {-x.v, -x.d}; }
NFS_HD nfs_d1 operator*(nfs_d1 x, nfs_d1 y) { return {x.v * y.v, x.d * y.v + x.v * y.d}; }
NFS_HD nfs_d1 operator/(nfs_d1 x, nfs_d1 y) {
    const double q = x.v / y.v;
    return {q, (x.d - q * y.d) / y.v};
}
// f(x) from f, f', f'' at x.v
NFS_HD nfs_d1 nfs_chain(nfs_d1 x, double f, double f1, double) { return {f, f1 * x.d}; }

NFS_HD nfs_d2 operator+(nfs_d2 x, nfs_d2 y) { return {x.v + y.v, x.a + y.a, x.b + y.b, x.ab + y.ab}; }
NFS_HD nfs_d2 operator-(nfs_d2 x, nfs_d2 y) { return {x.v - y.v, x.a - y.a, x.b - y.b, x.ab - y.ab}; }
NFS_HD nfs_d2 operator-(nfs_d2 x) { return {-x.v, -x.a, -x.b, -x.ab}; }
NFS_HD nfs_d2 operator*(nfs_d2 x, nfs_d2 y) {
    return {x.v * y.v, x.a * y.v + x.v * y.a, x.b * y.v + x.v * y.b, (x.ab * y.v + x.v * y.ab) + (x.a * y.b + x.b * y.a)};
}
NFS_HD nfs_d2 operator/(nfs_d2 x, nfs_d2 y) {                                // q y = x, differentiated twice
    const double q = x.v / y.v, qa = (x.a - q * y.a) / y.v, qb = (x.b - q * y.b) / y.v;
    return {q, qa, qb, (x.ab - ((qa * y.b + qb * y.a) + q * y.ab)) / y.v};
}
NFS_HD nfs_d2 nfs_chain(nfs_d2 x, double f, double f1, double f2) { return {f, f1 * x.a, f1 * x.b, f1 * x.ab + f2 * (x.a * x.b)}; }

template <class T> NFS_HD T nfs_sin(T x) { const double s = sin(x.v); return nfs_chain(x, s, cos(x.v), -s); }
template <class T> NFS_HD T nfs_cos(T x) { const double c = cos(x.v); return nfs_chain(x, c, -sin(x.v), -c); }
template <class T> NFS_HD T nfs_acos(T x) {                                  // |x.v| < 1
    const double w = 1.0 - x.v * x.v, r = sqrt(w);
    return nfs_chain(x, acos(x.v), -1.0 / r, -x.v / (w * r));
}
// torch.norm of a 3-vector: the square root of the sum of squares; at 0 the subgradient is 0, and so is every derivative of it
template <class T> NFS_HD T nfs_norm3(const T* x) {
    const T s = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    if (s.v == 0.0) return T(0.0);
    const double r = sqrt(s.v);
    return nfs_chain(s, r, 0.5 / r, -0.25 / (s.v * r));
}

template <class T> NFS_HD void nfs_matmul3(const T* A, const T* B, T* C) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[i * 3 + j] = (A[i * 3 + 0] * B[0 * 3 + j] + A[i * 3 + 1] * B[1 * 3 + j]) + A[i * 3 + 2] * B[2 * 3 + j];
}
template <class T> NFS_HD void nfs_hat(const T* k, T* K) {                   // skew_matrix (nav/math_utils.py:176-185)
    K[0] = T(0.0); K[1] = -k[2]; K[2] = k[1];
    K[3] = k[2]; K[4] = T(0.0); K[5] = -k[0];
    K[6] = -k[1]; K[7] = k[0]; K[8] = T(0.0);
}

// vec_to_rot_matrix (nav/math_utils.py:159-174): R = I + sin(a) K + ((1 - cos(a)) K) K, K = hat(r / (tiny + a)), a = |r|; `tiny` is the reference's 1e-10 in
// the precision the caller's route gives it
template <class T> NFS_HD void nfs_vec_to_rot(const T* r, double tiny, T* R) {
    const T a = nfs_norm3(r);
    const T d = T(tiny) + a;
    const T k[3] = {r[0] / d, r[1] / d, r[2] / d};
    T K[9], M[9], MK[9];
    nfs_hat(k, K);
    const T sn = nfs_sin(a), omc = T(1.0) - nfs_cos(a);
#pragma unroll
    for (int e = 0; e < 9; e++) M[e] = omc * K[e];
    nfs_matmul3(M, K, MK);
#pragma unroll
    for (int e = 0; e < 9; e++) R[e] = (T(e % 4 == 0 ? 1.0 : 0.0) + sn * K[e]) + MK[e];
}

// the axis part of measurement_fn's camera rotation (nav/estimator_helpers.py:301-309): P = cycle (rot_x(pi/2) R) diag(1, -1, -1); c90 is the reference's
// float32 cos((float)(pi / 2)), its sine is 1.  T = float is the filter's own pose chain (nav_filter.hip nf_pose)
template <class T> NFS_HD void nfs_camera_axes(const T* R, double c90, T* P) {
    T Rb[9];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        Rb[0 + j] = R[0 + j];
        Rb[3 + j] = T(c90) * R[3 + j] - R[6 + j];
        Rb[6 + j] = R[3 + j] + T(c90) * R[6 + j];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int m = (i + 1) % 3;
        P[i * 3 + 0] = Rb[m * 3 + 0]; P[i * 3 + 1] = -Rb[m * 3 + 1]; P[i * 3 + 2] = -Rb[m * 3 + 2];
    }
}
// measurement_fn's camera rotation as a function of the rotation vector, over forward-mode numbers
template <class T> NFS_HD void nfs_measurement_rotation(const T* r, double tiny, double c90, T* P) {
    T R[9];
    nfs_vec_to_rot(r, tiny, R);
    nfs_camera_axes(R, c90, P);
}

// Agent's cfg in double, with what the host prepares once: I^-1 (adjugate) and acos_safe's constants, eps = 1e-7, edge = acos(1 - eps), slope = edge / eps
struct nfs_dyn {
    double dt, mass, g, I[9], invI[9];
    double acos_eps, acos_lim, acos_edge, acos_edge_neg, acos_slope;
};

// rot_matrix_to_vec (nav/math_utils.py:116-157)
template <class T> NFS_HD void nfs_rot_to_vec(const nfs_dyn& D, const T* R, T* out) {
    const T trace = (R[0] + R[4]) + R[8];
    const T x = (trace - T(1.0)) / T(2.0);
    T angle;
    if (fabs(x.v) <= D.acos_lim) {
        angle = nfs_acos(x);
    } else {                                                                  // acos_safe's straight line beyond |x| = 1 - eps
        const double sg = x.v > 0.0 ? 1.0 : -1.0;
        const T ax = x.v > 0.0 ? x : -x;
        angle = T(sg > 0.0 ? D.acos_edge : D.acos_edge_neg) - T(D.acos_slope * sg) * ((ax - T(1.0)) + T(D.acos_eps));
    }
    if (angle.v == 0.0) {                                                    // vec[angle == 0] = 0: a constant; rot_vec = angle * vec
        out[0] = out[1] = out[2] = angle * T(0.0);
        return;
    }
    const T f = T(1.0) / (T(2.0) * nfs_sin(angle + T(1e-10)));
    const T w[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
#pragma unroll
    for (int i = 0; i < 3; i++) out[i] = angle * (f * w[i]);
}

// Agent.drone_dynamics (nav/agent_helpers.py:124-171): x = (position, velocity, rotation vector, body rate), action = (thrust, torque)
template <class T> NFS_HD void nfs_drone_dynamics(const nfs_dyn& D, const T* x, const double* action, T* next) {
    T R[9];
    nfs_vec_to_rot(x + 6, 1e-10, R);
    const T* om = x + 9;
    const double fz = action[0];
    T dv[3];
#pragma unroll
    for (int i = 0; i < 3; i++) dv[i] = (T(i == 2 ? -D.mass * D.g : 0.0) + R[i * 3 + 2] * T(fz)) / T(D.mass);
    T Iom[3], torque[3], domega[3];
#pragma unroll
    for (int i = 0; i < 3; i++) Iom[i] = (T(D.I[i * 3 + 0]) * om[0] + T(D.I[i * 3 + 1]) * om[1]) + T(D.I[i * 3 + 2]) * om[2];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        torque[i] = T(action[1 + i]) - (om[j] * Iom[k] - om[k] * Iom[j]);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) domega[i] = (T(D.invI[i * 3 + 0]) * torque[0] + T(D.invI[i * 3 + 1]) * torque[1]) + T(D.invI[i * 3 + 2]) * torque[2];
    // the exponential map of the angle displacement; theta == 0 gives the identity, a constant
    const T ang[3] = {om[0] * T(D.dt), om[1] * T(D.dt), om[2] * T(D.dt)};
    const T theta = nfs_norm3(ang);
    T Rn[9];
    if (theta.v == 0.0) {
#pragma unroll
        for (int e = 0; e < 9; e++) Rn[e] = R[e];
    } else {
        const T n[3] = {ang[0] / theta, ang[1] / theta, ang[2] / theta};
        T K[9], KK[9], E[9];
        nfs_hat(n, K);
        nfs_matmul3(K, K, KK);
        const T sn = nfs_sin(theta), omc = T(1.0) - nfs_cos(theta);
#pragma unroll
        for (int e = 0; e < 9; e++) E[e] = (T(e % 4 == 0 ? 1.0 : 0.0) + sn * K[e]) + omc * KK[e];
        nfs_matmul3(R, E, Rn);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        next[i] = x[i] + x[3 + i] * T(D.dt);
        next[3 + i] = x[3 + i] + dv[i] * T(D.dt);
        next[9 + i] = om[i] + domega[i] * T(D.dt);
    }
    nfs_rot_to_vec(D, Rn, next + 6);
}

// host: Agent's cfg as the C ABI carries it (float32) -> nfs_dyn.  0: fine; 1: dt or mass not finite or <= 0; 2: I singular (its determinant, taken in
// double, is 0 or not finite).  I^-1 is the adjugate over the determinant, in double.
inline int nfs_dyn_prepare(float dt, float mass, float g, const float* I, nfs_dyn& D) {
    if (!(isfinite(dt) && dt > 0.0f && isfinite(mass) && mass > 0.0f)) return 1;
    double a[9];
    for (int e = 0; e < 9; e++) a[e] = (double)I[e];
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
    const double det = (a[0] * c00 + a[1] * c01) + a[2] * c02;
    if (!(isfinite(det) && det != 0.0)) return 2;
    const double adj[9] = {c00, a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                           c01, a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                           c02, a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]};
    D.dt = (double)dt; D.mass = (double)mass; D.g = (double)g;
    for (int e = 0; e < 9; e++) { D.I[e] = a[e]; D.invI[e] = adj[e] / det; }
    D.acos_eps = 1e-7;
    D.acos_lim = 1.0 - D.acos_eps;
    D.acos_edge = acos(D.acos_lim);
    D.acos_edge_neg = acos(-D.acos_lim);
    D.acos_slope = D.acos_edge / D.acos_eps;
    return 0;
}
