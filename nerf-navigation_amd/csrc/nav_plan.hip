// nav_plan.hip -- the planner's optimisation epoch on the device (DESIGN.md §3.5 "Native planner"): Planner.calc_everything ->
// body_to_world -> get_state_cost -> total_cost -> backward -> Adam (nav/quad_plot.py:120-290) as three launches per epoch
// with no host synchronisation.
//
//   k_plan_kinematics   one workgroup: calc_everything forward from (states [R,4], initial_accel [2]) -> full states [S,18], actions [S,4],
//                       world points [S*B,3] = rot_i body_b + pos_i.                                     S = R + 3 trajectory rows
//   ngp_nav_density_value_jac (nav_field.hip, unchanged): sigma and d sigma / d x of the points, simulate.py:340's axis change folded in.
//   k_plan_cost_step    one workgroup: the forward again (in LDS), the cost, the gradient of total w.r.t. (initial_accel, states) and one
//                       step of torch.optim.Adam(capturable=True) on them.
//
// Gradient: forward-mode tangents, one lane per parameter.  The cost's adjoints are formed once per trajectory row (d total / d thrust_i,
// d total / d alpha_i, d total / d speed_i, and from sigma and its Jacobian g_i = sum_b d total / d p_ib, G_i = sum_b d total / d p_ib (x) body_b
// for the position and rotation of row i).  A parameter reaches rows t-4 .. t+1 only (t: the highest row whose position or rotation it
// moves; the duplicated last rows of acc and alpha are the +1), so a lane carries its tangent through those six rows in registers and
// contracts it with the adjoints.  The derivative conventions are torch autograd's (nav/math_utils.py:115-156): the linearised acos with
// its float32 slope, the 1 / (2 sin(ang + 1e-10)) factor, no gradient through a zero angle, zero gradient of the norm of a zero vector.
// No atomics; every sum runs in a fixed order, so two runs are bit-identical.
//
// Multi-start (DESIGN.md §3.5 "Multi-start planner"): ngp_plan_epochs_multi runs K trajectories of one objective as the SAME three launches per epoch.  The two
// one-workgroup kernels take a grid of K and workgroup k works on row k of every per-hypothesis buffer; the density query runs once over K S B points, each
// computed in its own lane.  So row k is the single run from the same start bit for bit.  k_plan_select keeps the best by the rule of ngp_select.h.
#include "ngp_nav_step.h"
#include "ngp_select.h"                                                   // ngp_select_best: the multi-start selection rule, shared with nav_filter.hip

#define NP_HD __host__ __device__ __forceinline__

static constexpr uint32_t NP_MIN_R = 2, NP_MAX_R = 255, NP_MAX_S = NP_MAX_R + 3;
static constexpr uint32_t NP_MAX_B = 65536;
static constexpr uint32_t NP_K1_THREADS = 1024, NP_K3_THREADS = 512;

// one trajectory row in LDS: forward values, then (cost step) the row's sums over its body points and its adjoints
enum : uint32_t {
    F_POS = 0, F_VEL = 3, F_ACC = 6, F_THR = 9, F_ROT = 10, F_XR = 19, F_XN = 22, F_HS = 23, F_HC = 24,
    F_X = 25, F_ANG = 26, F_C = 27, F_V = 28, F_VEC = 31, F_OM = 34, F_AL = 37, F_TQ = 40, F_TN = 43, F_SPD = 44,
    F_ATHR = 45, F_AAL = 46, F_ASP = 49, F_GP = 50, F_GR = 53, F_COLL = 62, F_PS = 63, NP_ROW = 64
};
static constexpr size_t NP_LDS = sizeof(float) * NP_ROW * NP_MAX_S;

struct np_args {
    uint32_t R, S, B;
    float dt, inv_dt, g, mass;
    float J[9], start[18], end[18];
    int32_t fade_out_epoch;
    float fade_out_sharpness;
    float acos_lim, acos_eps, acos_slope;           // (float)(1 - 1e-7), (float)1e-7, (float)(arccos(1 - 1e-7) / 1e-7) in float64
    ngp_adam_coef adam;
};

NP_HD void np_cross(const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

NP_HD float np_norm3(const float* a) { return sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }

// rows 0..3 and S-1: next_rotation (nav/quad_helpers.py:186-199) and the four positions fixed by the start state and initial_accel
NP_HD void np_head(const np_args& A, const float* ia, float* rows) {
    const float* s = A.start;
    const float* e = A.end;
    float phi[3] = {s[15] * A.dt, s[16] * A.dt, s[17] * A.dt};
    const float th = np_norm3(phi);
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    if (th != 0.0f) {
        const float k0 = phi[0] / th, k1 = phi[1] / th, k2 = phi[2] / th;
        const float K[9] = {0.f, -k2, k1, k2, 0.f, -k0, -k1, k0, 0.f};
        const float sn = sinf(th), cs = 1.0f - cosf(th);
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) {
                const float kk = K[a * 3 + 0] * K[0 * 3 + b] + K[a * 3 + 1] * K[1 * 3 + b] + K[a * 3 + 2] * K[2 * 3 + b];
                E[a * 3 + b] = (E[a * 3 + b] + sn * K[a * 3 + b]) + cs * kk;
            }
    }
    float* r0 = rows + F_ROT;
    float* rn = rows + NP_ROW + F_ROT;
    float* r1 = rows + (size_t)(A.S - 1) * NP_ROW + F_ROT;
#pragma unroll
    for (int k = 0; k < 9; k++) { r0[k] = s[6 + k]; r1[k] = e[6 + k]; }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++)
            rn[a * 3 + b] = r0[a * 3 + 0] * E[0 * 3 + b] + r0[a * 3 + 1] * E[1 * 3 + b] + r0[a * 3 + 2] * E[2 * 3 + b];
    const float grav[3] = {0.f, 0.f, -A.g};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float a_first = r0[a * 3 + 2] * ia[0] + grav[a];
        const float a_second = rn[a * 3 + 2] * ia[1] + grav[a];
        const float v_second = s[3 + a] + a_first * A.dt;
        const float v_third = v_second + a_second * A.dt;
        const float p_second = s[a] + s[3 + a] * A.dt;
        const float p_third = p_second + v_second * A.dt;
        rows[0 * NP_ROW + F_POS + a] = s[a];
        rows[1 * NP_ROW + F_POS + a] = p_second;
        rows[2 * NP_ROW + F_POS + a] = p_third;
        rows[3 * NP_ROW + F_POS + a] = p_third + v_third * A.dt;
        rows[(size_t)(A.S - 1) * NP_ROW + F_POS + a] = e[a];
    }
}

// rows 4 .. S-2: the decision positions states[2:, :3]
NP_HD void np_pos_row(const np_args& A, const float* states, float* rows, uint32_t i) {
#pragma unroll
    for (int a = 0; a < 3; a++) rows[(size_t)i * NP_ROW + F_POS + a] = states[(i - 2) * 4 + a];
}

NP_HD void np_vel_row(const np_args& A, float* rows, uint32_t i) {
    float* r = rows + (size_t)i * NP_ROW;
#pragma unroll
    for (int a = 0; a < 3; a++) r[F_VEL + a] = i + 1 < A.S ? (r[NP_ROW + F_POS + a] - r[F_POS + a]) * A.inv_dt : A.end[3 + a];
}

// acceleration (the last row repeats row S-2), thrust, speed and, for rows 2 .. S-2, the rotation from the thrust axis and the heading
NP_HD void np_acc_row(const np_args& A, const float* states, float* rows, uint32_t i) {
    float* r = rows + (size_t)i * NP_ROW;
    const float* src = rows + (size_t)(i + 1 < A.S ? i : A.S - 2) * NP_ROW;
    const float grav[3] = {0.f, 0.f, -A.g};
    float acc[3];
#pragma unroll
    for (int a = 0; a < 3; a++) acc[a] = (src[NP_ROW + F_VEL + a] - src[F_VEL + a]) * A.inv_dt - grav[a];
    const float thr = np_norm3(acc);
#pragma unroll
    for (int a = 0; a < 3; a++) r[F_ACC + a] = acc[a];
    r[F_THR] = thr;
    const float* v = r + F_VEL;
    r[F_SPD] = sqrtf(((v[0] * v[0] + 1e-5f) + (v[1] * v[1] + 1e-5f)) + (v[2] * v[2] + 1e-5f));
    if (i < 2 || i + 1 >= A.S) return;
    const float zb[3] = {acc[0] / thr, acc[1] / thr, acc[2] / thr};
    const float h = states[(i - 2) * 4 + 3];
    const float hs = sinf(h), hc = cosf(h);
    const float pl[3] = {hs, -hc, 0.0f};
    float xr[3], xb[3], yb[3];
    np_cross(zb, pl, xr);
    const float xn = np_norm3(xr);
#pragma unroll
    for (int a = 0; a < 3; a++) xb[a] = xr[a] / xn;
    np_cross(zb, xb, yb);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        r[F_ROT + a * 3 + 0] = xb[a];
        r[F_ROT + a * 3 + 1] = yb[a];
        r[F_ROT + a * 3 + 2] = zb[a];
        r[F_XR + a] = xr[a];
    }
    r[F_XN] = xn; r[F_HS] = hs; r[F_HC] = hc;
}

// omega_i = rot_matrix_to_vec(rot_{i+1} rot_i^T) / dt (nav/math_utils.py:115-156); the last row is the end state's rate
NP_HD void np_log_row(const np_args& A, float* rows, uint32_t i) {
    float* r = rows + (size_t)i * NP_ROW;
    if (i + 1 >= A.S) {
#pragma unroll
        for (int a = 0; a < 3; a++) r[F_OM + a] = A.end[15 + a];
        return;
    }
    const float* r0 = r + F_ROT;
    const float* r1 = r + NP_ROW + F_ROT;
    float M[9];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++)
            M[a * 3 + b] = (r1[a * 3 + 0] * r0[b * 3 + 0] + r1[a * 3 + 1] * r0[b * 3 + 1]) + r1[a * 3 + 2] * r0[b * 3 + 2];
    const float tr = (M[0] + M[4]) + M[8];
    const float x = (tr - 1.0f) * 0.5f;
    float ang;
    if (fabsf(x) <= A.acos_lim) {
        ang = acosf(x);
    } else {
        const float sg = x > 0.0f ? 1.0f : -1.0f;
        ang = acosf(sg * A.acos_lim) - (A.acos_slope * sg) * ((fabsf(x) - 1.0f) + A.acos_eps);
    }
    const float c = 1.0f / (2.0f * sinf(ang + 1e-10f));
    const float v[3] = {M[7] - M[5], M[2] - M[6], M[3] - M[1]};
    r[F_X] = x; r[F_ANG] = ang; r[F_C] = c;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float vec = ang == 0.0f ? 0.0f : c * v[a];
        r[F_V + a] = v[a];
        r[F_VEC + a] = vec;
        r[F_OM + a] = (ang * vec) * A.inv_dt;
    }
}

// angular acceleration (the last row repeats row S-2), torque = J alpha and its norm
NP_HD void np_alpha_row(const np_args& A, float* rows, uint32_t i) {
    float* r = rows + (size_t)i * NP_ROW;
    const float* src = rows + (size_t)(i + 1 < A.S ? i : A.S - 2) * NP_ROW;
    float al[3];
#pragma unroll
    for (int a = 0; a < 3; a++) al[a] = (src[NP_ROW + F_OM + a] - src[F_OM + a]) * A.inv_dt;
    float tq[3];
#pragma unroll
    for (int a = 0; a < 3; a++) tq[a] = (A.J[a * 3 + 0] * al[0] + A.J[a * 3 + 1] * al[1]) + A.J[a * 3 + 2] * al[2];
#pragma unroll
    for (int a = 0; a < 3; a++) { r[F_AL + a] = al[a]; r[F_TQ + a] = tq[a]; }
    r[F_TN] = np_norm3(tq);
}

// element e of the world points [S*B,3]: rot_i body_b + pos_i (body_to_world, nav/quad_plot.py:216-222)
NP_HD float np_point(const np_args& A, const float* rows, const float* body, uint32_t e) {
    const uint32_t ib = e / 3, a = e - 3 * ib, i = ib / A.B, b = ib - i * A.B;
    const float* r = rows + (size_t)i * NP_ROW;
    const float* bb = body + 3 * (size_t)b;
    return ((r[F_ROT + a * 3 + 0] * bb[0] + r[F_ROT + a * 3 + 1] * bb[1]) + r[F_ROT + a * 3 + 2] * bb[2]) + r[F_POS + a];
}

// the fade-out mask of get_state_cost (nav/quad_plot.py:243-247): torch.linspace(0, 1, S) in float32, sigmoid in float32
NP_HD float np_mask(const np_args& A, uint32_t epoch, uint32_t i) {
    if (!((int64_t)epoch < (int64_t)A.fade_out_epoch)) return 1.0f;
    const float step = 1.0f / (float)(A.S - 1);
    const float t = i < A.S / 2 ? step * (float)i : 1.0f - step * (float)(A.S - 1 - i);
    const float position = (float)((double)epoch / (double)A.fade_out_epoch);
    const float z = A.fade_out_sharpness * (position - t);
    return 1.0f / (1.0f + expf(-z));
}

// row i's cost and adjoints, from its sums over the body points: F_COLL = sum_b sigma^2 speed, F_ASP = sum_b sigma^2,
// F_GP = sum_b 2 sigma dsigma/dx, F_GR = sum_b 2 sigma dsigma/dx (x) body_b
NP_HD void np_row_cost(const np_args& A, float* rows, uint32_t i, uint32_t epoch) {
    float* r = rows + (size_t)i * NP_ROW;
    const float mask = np_mask(A, epoch, i);
    const float inv_S = 1.0f / (float)A.S, inv_B = 1.0f / (float)A.B;
    const float coll = (r[F_COLL] * inv_B) * mask;
    const float thr_m = r[F_THR] * A.mass;
    const float tn = r[F_TN];
    const float tn2 = tn * tn;
    r[F_PS] = (1000.0f * (thr_m * thr_m) + 0.01f * (tn2 * tn2)) + coll * 1e6f;
    r[F_COLL] = coll * 1e6f;
    r[F_ATHR] = inv_S * 1000.0f * 2.0f * thr_m * A.mass;
    float k = inv_S * 0.04f * tn2;                                      // d(0.01 |tq|^4)/d tq = 0.04 |tq|^2 tq
    float gtq[3];
#pragma unroll
    for (int a = 0; a < 3; a++) gtq[a] = k * r[F_TQ + a];
#pragma unroll
    for (int m = 0; m < 3; m++) r[F_AAL + m] = (A.J[0 * 3 + m] * gtq[0] + A.J[1 * 3 + m] * gtq[1]) + A.J[2 * 3 + m] * gtq[2];
    const float ks = inv_S * 1e6f * mask * inv_B;
    r[F_ASP] = ks * r[F_ASP];
    const float kp = ks * r[F_SPD];
#pragma unroll
    for (int a = 0; a < 3; a++) r[F_GP + a] *= kp;
#pragma unroll
    for (int a = 0; a < 9; a++) r[F_GR + a] *= kp;
}

// d total / d parameter p (0, 1: initial_accel; 2 + 4 r + c: states[r][c]) by one forward-mode tangent through rows t-4 .. t+1
NP_HD float np_tangent(const np_args& A, const float* rows, uint32_t p) {
    const int S = (int)A.S;
    int t;
    float dh = 0.0f;
    float dp[6][3];
#pragma unroll
    for (int j = 0; j < 6; j++)
#pragma unroll
        for (int a = 0; a < 3; a++) dp[j][a] = 0.0f;
    if (p < 2) {                                                          // p_third, p_fourth (rows 2, 3) through a_first / a_second
        t = 3;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float ez0 = rows[0 * NP_ROW + F_ROT + a * 3 + 2], ezn = rows[1 * NP_ROW + F_ROT + a * 3 + 2];
            const float dvs = p == 0 ? ez0 * A.dt : 0.0f;
            const float dvt = p == 0 ? dvs : ezn * A.dt;
            const float dp3 = dvs * A.dt;
            dp[3][a] = dp3;
            dp[4][a] = dp3 + dvt * A.dt;
        }
    } else {
        const uint32_t q = p - 2, rr = q / 4, c = q - 4 * rr;
        t = (int)rr + 2;
        if (c == 3) dh = 1.0f;
        else if (rr < 2) return 0.0f;                                     // states[0:2, :3] are not used (nav/quad_plot.py:148)
        else {
#pragma unroll
            for (int a = 0; a < 3; a++) dp[4][a] = a == (int)c ? 1.0f : 0.0f;
        }
    }
    float dv[6][3], da[6][3], dthr[6], drot[6][9], dom[6][3], dal[6][3];
#pragma unroll
    for (int j = 0; j < 6; j++) {                                         // velocity
        const int i = t - 4 + j;
        const bool in = i >= 0 && i <= S - 2;
#pragma unroll
        for (int a = 0; a < 3; a++) dv[j][a] = in ? ((j < 5 ? dp[j + 1][a] : 0.0f) - dp[j][a]) * A.inv_dt : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 6; j++) {                                         // acceleration, thrust, rotation
        const int i = t - 4 + j;
        const float* r = rows + (size_t)(i < 0 ? 0 : i) * NP_ROW;
#pragma unroll
        for (int a = 0; a < 3; a++)
            da[j][a] = (i == S - 1 && j > 0) ? da[j - 1][a] : (i >= 0 && i <= S - 2 ? ((j < 5 ? dv[j + 1][a] : 0.0f) - dv[j][a]) * A.inv_dt : 0.0f);
        dthr[j] = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; k++) drot[j][k] = 0.0f;
        if (i < 0 || i > S - 1) continue;
        const float thr = r[F_THR];
        dthr[j] = thr == 0.0f ? 0.0f : ((r[F_ACC] * da[j][0] + r[F_ACC + 1] * da[j][1]) + r[F_ACC + 2] * da[j][2]) / thr;
        const float dhj = j == 4 ? dh : 0.0f;
        if (i < 2 || i > S - 2) continue;
        float zb[3], xb[3], dzb[3], dxr[3], dxb[3], dyb[3], tmp[3], tmp2[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            zb[a] = r[F_ROT + a * 3 + 2];
            xb[a] = r[F_ROT + a * 3 + 0];
            dzb[a] = da[j][a] / thr - r[F_ACC + a] * dthr[j] / (thr * thr);
        }
        const float pl[3] = {r[F_HS], -r[F_HC], 0.0f};
        const float dpl[3] = {r[F_HC] * dhj, r[F_HS] * dhj, 0.0f};
        np_cross(dzb, pl, tmp);
        np_cross(zb, dpl, tmp2);
#pragma unroll
        for (int a = 0; a < 3; a++) dxr[a] = tmp[a] + tmp2[a];
        const float xn = r[F_XN];
        const float dxn = xn == 0.0f ? 0.0f : ((r[F_XR] * dxr[0] + r[F_XR + 1] * dxr[1]) + r[F_XR + 2] * dxr[2]) / xn;
#pragma unroll
        for (int a = 0; a < 3; a++) dxb[a] = dxr[a] / xn - r[F_XR + a] * dxn / (xn * xn);
        np_cross(dzb, xb, tmp);
        np_cross(zb, dxb, tmp2);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            dyb[a] = tmp[a] + tmp2[a];
            drot[j][a * 3 + 0] = dxb[a];
            drot[j][a * 3 + 1] = dyb[a];
            drot[j][a * 3 + 2] = dzb[a];
        }
    }
#pragma unroll
    for (int j = 0; j < 6; j++) {                                         // omega through the log map
        const int i = t - 4 + j;
#pragma unroll
        for (int a = 0; a < 3; a++) dom[j][a] = 0.0f;
        if (i < 0 || i > S - 2) continue;
        const float* r = rows + (size_t)i * NP_ROW;
        const float ang = r[F_ANG];
        if (ang == 0.0f) continue;                                        // overwritten by zero: no gradient (nav/math_utils.py:150)
        const float* r0 = r + F_ROT;
        const float* r1 = r + NP_ROW + F_ROT;
        float dM[9];
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) {
                float s = 0.0f;
#pragma unroll
                for (int k = 0; k < 3; k++) s += (j < 5 ? drot[j + 1][a * 3 + k] : 0.0f) * r0[b * 3 + k] + r1[a * 3 + k] * drot[j][b * 3 + k];
                dM[a * 3 + b] = s;
            }
        const float dx = ((dM[0] + dM[4]) + dM[8]) * 0.5f;
        const float x = r[F_X], c = r[F_C];
        const float dang = fabsf(x) <= A.acos_lim ? -dx / sqrtf(1.0f - x * x) : -A.acos_slope * dx;
        const float dc = -(c * c) * (2.0f * cosf(ang + 1e-10f) * dang);
        const float dvv[3] = {dM[7] - dM[5], dM[2] - dM[6], dM[3] - dM[1]};
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float dvec = dc * r[F_V + a] + c * dvv[a];
            dom[j][a] = (dang * r[F_VEC + a] + ang * dvec) * A.inv_dt;
        }
    }
    float grad = 0.0f;
#pragma unroll
    for (int j = 0; j < 6; j++) {                                         // angular acceleration, speed; contraction with the adjoints
        const int i = t - 4 + j;
#pragma unroll
        for (int a = 0; a < 3; a++)
            dal[j][a] = (i == S - 1 && j > 0) ? dal[j - 1][a] : (i >= 0 && i <= S - 2 ? ((j < 5 ? dom[j + 1][a] : 0.0f) - dom[j][a]) * A.inv_dt : 0.0f);
        if (i < 0 || i > S - 1) continue;
        const float* r = rows + (size_t)i * NP_ROW;
        float g = r[F_ATHR] * dthr[j];
#pragma unroll
        for (int a = 0; a < 3; a++) g += r[F_AAL + a] * dal[j][a];
        if (i <= S - 2) {
            const float dsp = ((r[F_VEL] * dv[j][0] + r[F_VEL + 1] * dv[j][1]) + r[F_VEL + 2] * dv[j][2]) / r[F_SPD];
            g += r[F_ASP] * dsp;
#pragma unroll
            for (int a = 0; a < 3; a++) g += r[F_GP + a] * dp[j][a];
#pragma unroll
            for (int k = 0; k < 9; k++) g += r[F_GR + k] * drot[j][k];
        }
        grad += g;
    }
    return grad;
}

// ---------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------

__device__ void np_forward(const np_args& A, const float* __restrict__ states, const float* __restrict__ ia, float* rows) {
    const uint32_t tid = threadIdx.x, NT = blockDim.x;
    if (tid == 0) np_head(A, ia, rows);
    for (uint32_t i = 4 + tid; i + 1 < A.S; i += NT) np_pos_row(A, states, rows, i);
    __syncthreads();
    for (uint32_t i = tid; i < A.S; i += NT) np_vel_row(A, rows, i);
    __syncthreads();
    for (uint32_t i = tid; i < A.S; i += NT) np_acc_row(A, states, rows, i);
    __syncthreads();
    for (uint32_t i = tid; i < A.S; i += NT) np_log_row(A, rows, i);
    __syncthreads();
    for (uint32_t i = tid; i < A.S; i += NT) np_alpha_row(A, rows, i);
    __syncthreads();
}

// Both kernels serve one hypothesis per workgroup: workgroup k = blockIdx.x owns row k of every per-hypothesis buffer (states [K,R,4], initial_accel
// [K,2], adam [K,3P+1], points [K,S*B,3], sigma [K,S*B], jac [K,S*B,3], loss [K], per_state [K,2,S], full [K,S,18], actions [K,S,4]): the kernels offset the
// pointers (in size_t) and run the bodies np_kinematics / np_cost_step, which keep their __restrict__ arguments.  The single entry points launch a grid of 1,
// where every offset is zero.
__device__ __forceinline__ void np_kinematics(const np_args& A, const float* __restrict__ states, const float* __restrict__ ia,
                                              const float* __restrict__ body, float* __restrict__ full, float* __restrict__ actions,
                                              float* __restrict__ points) {
    extern __shared__ float rows[];
    np_forward(A, states, ia, rows);
    const uint32_t tid = threadIdx.x, NT = blockDim.x;
    if (full)                                                             // get_full_states: pos, vel, rot (row-major), omega
        for (uint32_t e = tid; e < 18 * A.S; e += NT) {
            const uint32_t i = e / 18, k = e - 18 * i;
            const float* r = rows + (size_t)i * NP_ROW;
            full[e] = k < 3 ? r[F_POS + k] : k < 6 ? r[F_VEL + k - 3] : k < 15 ? r[F_ROT + k - 6] : r[F_OM + k - 15];
        }
    if (actions)                                                          // thrust * mass, torque
        for (uint32_t e = tid; e < 4 * A.S; e += NT) {
            const uint32_t i = e / 4, k = e - 4 * i;
            const float* r = rows + (size_t)i * NP_ROW;
            actions[e] = k == 0 ? r[F_THR] * A.mass : r[F_TQ + k - 1];
        }
    if (points)
        for (uint32_t e = tid; e < 3 * A.S * A.B; e += NT) points[e] = np_point(A, rows, body, e);
}

__global__ __launch_bounds__(NP_K1_THREADS) void k_plan_kinematics(np_args A, const float* states, const float* ia, const float* body, float* full,
                                                                   float* actions, float* points) {
    const size_t k = blockIdx.x;
    np_kinematics(A, states + k * 4 * (size_t)A.R, ia + k * 2, body, full ? full + k * 18 * (size_t)A.S : nullptr,
                  actions ? actions + k * 4 * (size_t)A.S : nullptr, points ? points + k * 3 * (size_t)A.S * A.B : nullptr);
}

__device__ __forceinline__ void np_cost_step(const np_args& Aarg, uint32_t epoch, int update, float* __restrict__ states, float* __restrict__ ia,
                                             float* __restrict__ adam, const float* __restrict__ body, const float* __restrict__ sigma,
                                             const float* __restrict__ jac, float* __restrict__ loss, float* __restrict__ per_state) {
    extern __shared__ float rows[];
    __shared__ np_args A;                                                 // the arguments from LDS: held in SGPRs they spill
    const uint32_t tid = threadIdx.x, NT = blockDim.x, P = 4 * Aarg.R + 2;
    if (tid == 0) A = Aarg;
    const float step = adam[3 * P] + 1.0f;                                // read before any lane writes it (there are barriers in between)
    __syncthreads();
    np_forward(A, states, ia, rows);
    // each row's sums over its body points: one wave per row, lanes strided over the points, then a fixed butterfly
    const uint32_t lane = tid & 63, wave = tid >> 6, NW = NT >> 6;
    for (uint32_t i = wave; i < A.S; i += NW) {
        float* r = rows + (size_t)i * NP_ROW;
        const float spd = r[F_SPD];
        float sc = 0.0f, s2 = 0.0f, gp[3] = {0.f, 0.f, 0.f}, gr[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (uint32_t b = lane; b < A.B; b += 64) {
            const size_t n = (size_t)i * A.B + b;
            const float sg = sigma[n];
            const float d = sg * sg;
            sc += d * spd;
            s2 += d;
            const float w = 2.0f * sg;
            const float q[3] = {w * jac[3 * n], w * jac[3 * n + 1], w * jac[3 * n + 2]};
            const float bb[3] = {body[3 * b], body[3 * b + 1], body[3 * b + 2]};
#pragma unroll
            for (int a = 0; a < 3; a++) {
                gp[a] += q[a];
#pragma unroll
                for (int m = 0; m < 3; m++) gr[a * 3 + m] += q[a] * bb[m];
            }
        }
        sc = ngp_wave_sum(sc);
        s2 = ngp_wave_sum(s2);
#pragma unroll
        for (int a = 0; a < 3; a++) gp[a] = ngp_wave_sum(gp[a]);
#pragma unroll
        for (int k = 0; k < 9; k++) gr[k] = ngp_wave_sum(gr[k]);
        if (lane == 0) {
            r[F_COLL] = sc;
            r[F_ASP] = s2;
#pragma unroll
            for (int a = 0; a < 3; a++) r[F_GP + a] = gp[a];
#pragma unroll
            for (int k = 0; k < 9; k++) r[F_GR + k] = gr[k];
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < A.S; i += NT) np_row_cost(A, rows, i, epoch);
    __syncthreads();
    if (tid == 0) {
        float total = 0.0f;
        for (uint32_t i = 0; i < A.S; i++) total += rows[(size_t)i * NP_ROW + F_PS];
        if (loss) *loss = total / (float)A.S;
    }
    if (per_state)
        for (uint32_t i = tid; i < A.S; i += NT) {
            per_state[i] = rows[(size_t)i * NP_ROW + F_PS];
            per_state[A.S + i] = rows[(size_t)i * NP_ROW + F_COLL];
        }
    for (uint32_t p = tid; p < P; p += NT) {
        const float g = np_tangent(A, rows, p);
        adam[2 * P + p] = g;
        if (update) {
            float* param = p < 2 ? ia + p : states + (p - 2);
            float m = adam[p], v = adam[P + p];
            *param = ngp_adam_step(A.adam, *param, g, &m, &v, step);
            adam[p] = m;
            adam[P + p] = v;
        }
    }
    if (update && tid == 0) adam[3 * P] = step;
}

__global__ __launch_bounds__(NP_K3_THREADS) void k_plan_cost_step(np_args A, uint32_t epoch, int update, float* states, float* ia, float* adam,
                                                                  const float* body, const float* sigma, const float* jac, float* loss, float* per_state) {
    const size_t k = blockIdx.x, M = (size_t)A.S * A.B, P = 4 * (size_t)A.R + 2;
    np_cost_step(A, epoch, update, states + k * 4 * (size_t)A.R, ia + k * 2, adam + k * (3 * P + 1), body, sigma + k * M, jac + k * 3 * M,
                 loss ? loss + k : nullptr, per_state ? per_state + k * 2 * (size_t)A.S : nullptr);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

// workspace (256-byte aligned pieces): body points of every state [(R + 3) B][3] | their density | its Jacobian [..][3]
// K hypotheses: the same three pieces for K (R + 3) B points, hypothesis k in [k S B, (k + 1) S B); one statement for both entry points, K = 1 is the single loop's.
// K S B <= 2^26 keeps the point count and the kernels' 3x element indices inside uint32_t (every R, B of the single path passes at K = 1: 258 * 65536 < 2^25)
struct np_ws { float* points; float* sigma; float* jac; size_t total; };
static constexpr uint64_t NP_MAX_POINTS = 1ull << 26;
static np_ws np_multi_layout(uint32_t K, uint32_t R, uint32_t B, void* base) {
    if (K < 1 || K > NGP_PLAN_MULTI_MAX_K || R < NP_MIN_R || R > NP_MAX_R || B < 1 || B > NP_MAX_B || (uint64_t)K * (R + 3) * B > NP_MAX_POINTS)
        return {};                                                                 // total 0: a shape no planner call accepts
    const size_t n = (size_t)K * (R + 3) * B;
    ngp_carver c(base);
    return {c.take<float>(3 * n), c.take<float>(n), c.take<float>(3 * n), c.total(256)};
}
static np_ws np_layout(uint32_t R, uint32_t B, void* base) { return np_multi_layout(1, R, B, base); }
extern "C" size_t ngp_plan_workspace(uint32_t R, uint32_t B) { return np_layout(R, B, nullptr).total; }
extern "C" size_t ngp_plan_multi_workspace(uint32_t K, uint32_t R, uint32_t B) { return np_multi_layout(K, R, B, nullptr).total; }

static int np_fill(const char* who, const ngp_plan_cfg_t* c, uint32_t R, uint32_t B, np_args& A) {
    NGP_REQUIRE(c, "%s: null cfg", who);
    NGP_REQUIRE(R >= NP_MIN_R && R <= NP_MAX_R, "%s: R = %u rows of states; supported 2 <= R <= 255", who, R);
    NGP_REQUIRE(B >= 1 && B <= NP_MAX_B, "%s: B = %u body points; supported 1 <= B <= 65536", who, B);
    NGP_REQUIRE(c->dt > 0.0f, "%s: dt must be positive", who);
    A.R = R; A.S = R + 3; A.B = B;
    A.dt = c->dt; A.inv_dt = 1.0f / c->dt; A.g = c->g; A.mass = c->mass;
#pragma unroll
    for (int k = 0; k < 9; k++) A.J[k] = c->J[k];
#pragma unroll
    for (int k = 0; k < 18; k++) { A.start[k] = c->start[k]; A.end[k] = c->end[k]; }
    A.fade_out_epoch = c->fade_out_epoch;
    A.fade_out_sharpness = c->fade_out_sharpness;
    const double eps = 1e-7;
    A.acos_lim = (float)(1.0 - eps);
    A.acos_eps = (float)eps;
    A.acos_slope = (float)(acos(1.0 - eps) / eps);
    A.adam = ngp_adam_fill(c->lr, c->beta1, c->beta2, c->eps);
    return NGP_OK;
}

// the kernels keep all S <= 258 rows in LDS (66 KB): above the default dynamic limit, raised once per device
static int np_allow_lds() {
    static std::atomic<unsigned long long> devices{0};
    const int rc = ngp_allow_dynamic_lds(devices, {(const void*)k_plan_kinematics, (const void*)k_plan_cost_step}, NP_LDS);
    if (rc == NGP_LDS_NO_DEVICE) return ngp_fail(NGP_ELAUNCH, "plan: no current device");
    if (rc != NGP_LDS_OK) return ngp_fail(NGP_ELAUNCH, "plan: cannot raise the dynamic LDS limit");
    return NGP_OK;
}

static size_t np_lds(uint32_t S) { return sizeof(float) * NP_ROW * S; }

extern "C" int ngp_plan_kinematics(const ngp_plan_cfg_t* cfg, const float* states, const float* initial_accel, uint32_t R,
                                   const float* body, uint32_t B, float* full_states, float* actions, float* points, void* stream) {
    np_args A;
    const int rc = np_fill("plan_kinematics", cfg, R, points ? B : 1u, A);
    if (rc != NGP_OK) return rc;
    NGP_REQUIRE(states && initial_accel, "plan_kinematics: null states / initial_accel");
    NGP_REQUIRE(!points || body, "plan_kinematics: points need the body");
    { const int rc_lds = np_allow_lds(); if (rc_lds != NGP_OK) return rc_lds; }
    hipLaunchKernelGGL(k_plan_kinematics, dim3(1), dim3(NP_K1_THREADS), np_lds(A.S), (hipStream_t)stream, A, states, initial_accel, body,
                       full_states, actions, points);
    NGP_CHECK_LAUNCH("plan_kinematics");
    return NGP_OK;
}

// the loop of both entry points, after the shape (A) has been accepted: the null-pointer refusal, the workspace (whose size function `ws_fn` names), the
// field, then per epoch three launches whatever K is -- the kinematics and the cost step with a grid of K, the density query once over K S B points.
// losses [n_epochs,K], per_state [K,2,S]
static int np_epochs(const char* who, const char* ws_fn, const np_args& A, const ngp_nav_field_t* field, const void* prepared, const ngp_plan_cfg_t* cfg,
                     uint32_t K, float* states, float* initial_accel, float* adam_states, const float* body, uint32_t first_epoch, uint32_t n_epochs,
                     int update, float* losses, float* per_state, void* workspace, size_t workspace_bytes, void* stream) {
    NGP_REQUIRE(states && initial_accel && adam_states && body, "%s: null pointer", who);
    const np_ws w = np_multi_layout(K, A.R, A.B, workspace);
    if (!workspace || workspace_bytes < w.total)
        return ngp_fail(NGP_EWORKSPACE, "%s: workspace of %zu bytes, needs %s = %zu", who, workspace_bytes, ws_fn, w.total);
    const uint32_t M = K * A.S * A.B;                                      // <= 2^26 (np_multi_layout)
    float* points = w.points, *sigma = w.sigma, *jac = w.jac;
    {   // the field is checked here, before anything is queued (M = 0 validates and launches nothing)
        const int rc_f = ngp_nav_density_value_jac(field, prepared, points, 0, cfg->rot, sigma, jac, stream);
        if (rc_f != NGP_OK) return rc_f;
    }
    if (n_epochs == 0) return NGP_OK;
    { const int rc_lds = np_allow_lds(); if (rc_lds != NGP_OK) return rc_lds; }
    const size_t lds = np_lds(A.S);
    for (uint32_t k = 0; k < n_epochs; k++) {
        hipLaunchKernelGGL(k_plan_kinematics, dim3(K), dim3(NP_K1_THREADS), lds, (hipStream_t)stream, A, (const float*)states,
                           (const float*)initial_accel, body, (float*)nullptr, (float*)nullptr, points);
        { const hipError_t e = hipGetLastError(); if (e != hipSuccess) return ngp_fail(NGP_ELAUNCH, "%s: kinematics: %s", who, hipGetErrorString(e)); }
        const int rc_q = ngp_nav_density_value_jac(field, prepared, points, M, cfg->rot, sigma, jac, stream);
        if (rc_q != NGP_OK) return rc_q;
        hipLaunchKernelGGL(k_plan_cost_step, dim3(K), dim3(NP_K3_THREADS), lds, (hipStream_t)stream, A, first_epoch + k, update, states,
                           initial_accel, adam_states, body, (const float*)sigma, (const float*)jac,
                           losses ? losses + (size_t)k * K : (float*)nullptr, k + 1 == n_epochs ? per_state : (float*)nullptr);
        { const hipError_t e = hipGetLastError(); if (e != hipSuccess) return ngp_fail(NGP_ELAUNCH, "%s: cost step: %s", who, hipGetErrorString(e)); }
    }
    return NGP_OK;
}

extern "C" int ngp_plan_epochs(const ngp_nav_field_t* field, const void* prepared, const ngp_plan_cfg_t* cfg, float* states,
                               float* initial_accel, float* adam_state, const float* body, uint32_t B, uint32_t R, uint32_t first_epoch,
                               uint32_t n_epochs, int update, float* losses, float* per_state, void* workspace, size_t workspace_bytes,
                               void* stream) {
    np_args A;
    const int rc = np_fill("plan_epochs", cfg, R, B, A);
    if (rc != NGP_OK) return rc;
    return np_epochs("plan_epochs", "ngp_plan_workspace(R, B)", A, field, prepared, cfg, 1, states, initial_accel, adam_state, body, first_epoch, n_epochs,
                     update, losses, per_state, workspace, workspace_bytes, stream);
}

extern "C" int ngp_plan_epochs_multi(const ngp_nav_field_t* field, const void* prepared, const ngp_plan_cfg_t* cfg, uint32_t K, float* states,
                                     float* initial_accel, float* adam_states, const float* body, uint32_t B, uint32_t R, uint32_t first_epoch,
                                     uint32_t n_epochs, int update, float* losses, float* per_state, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    NGP_REQUIRE(K >= 1 && K <= NGP_PLAN_MULTI_MAX_K, "plan_epochs_multi: K = %u hypotheses; supported 1 <= K <= %u", K, NGP_PLAN_MULTI_MAX_K);
    np_args A;
    const int rc = np_fill("plan_epochs_multi", cfg, R, B, A);
    if (rc != NGP_OK) return rc;
    NGP_REQUIRE((uint64_t)K * A.S * B <= NP_MAX_POINTS, "plan_epochs_multi: K * S * B = %u * %u * %u body points per epoch; supported K * S * B <= 2^26", K,
                A.S, B);
    return np_epochs("plan_epochs_multi", "ngp_plan_multi_workspace(K, R, B)", A, field, prepared, cfg, K, states, initial_accel, adam_states, body,
                     first_epoch, n_epochs, update, losses, per_state, workspace, workspace_bytes, stream);
}

// one workgroup: every lane scans the K losses (K <= 64) by the rule of ngp_select.h, the lanes copy the winner's 4 R states and 2 accelerations, lane 0 its
// loss and index
static constexpr uint32_t NP_SELECT_THREADS = 256;
__global__ __launch_bounds__(NP_SELECT_THREADS) void k_plan_select(const float* __restrict__ losses, const float* __restrict__ states,
                                                                   const float* __restrict__ ia, uint32_t K, uint32_t R, float* __restrict__ best_states,
                                                                   float* __restrict__ best_accel, float* __restrict__ best_loss,
                                                                   uint32_t* __restrict__ best_index) {
    const uint32_t best = ngp_select_best(losses, K);
    const float* src = states + 4 * (size_t)R * best;
    for (uint32_t e = threadIdx.x; e < 4 * R; e += blockDim.x) best_states[e] = src[e];
    if (threadIdx.x < 2) best_accel[threadIdx.x] = ia[2 * (size_t)best + threadIdx.x];
    if (threadIdx.x == 0) { *best_loss = losses[best]; *best_index = best; }
}

static int np_select_args(const char* who, const float* losses, const float* states, const float* initial_accel, uint32_t K, uint32_t R,
                          float* best_states, float* best_accel, float* best_loss, uint32_t* best_index) {
    NGP_REQUIRE(K >= 1 && K <= NGP_PLAN_MULTI_MAX_K, "%s: K = %u hypotheses; supported 1 <= K <= %u", who, K, NGP_PLAN_MULTI_MAX_K);
    NGP_REQUIRE(R >= NP_MIN_R && R <= NP_MAX_R, "%s: R = %u rows of states; supported 2 <= R <= 255", who, R);
    NGP_REQUIRE(losses && states && initial_accel && best_states && best_accel && best_loss && best_index, "%s: null pointer", who);
    return NGP_OK;
}

extern "C" int ngp_plan_select(const float* losses, const float* states, const float* initial_accel, uint32_t K, uint32_t R, float* best_states,
                               float* best_accel, float* best_loss, uint32_t* best_index, void* stream) {
    const int rc = np_select_args("plan_select", losses, states, initial_accel, K, R, best_states, best_accel, best_loss, best_index);
    if (rc != NGP_OK) return rc;
    hipLaunchKernelGGL(k_plan_select, dim3(1), dim3(NP_SELECT_THREADS), 0, (hipStream_t)stream, losses, states, initial_accel, K, R, best_states, best_accel,
                       best_loss, best_index);
    NGP_CHECK_LAUNCH("plan_select");
    return NGP_OK;
}

extern "C" int ngp_plan_select_host(const float* losses, const float* states, const float* initial_accel, uint32_t K, uint32_t R, float* best_states,
                                    float* best_accel, float* best_loss, uint32_t* best_index) {
    const int rc = np_select_args("plan_select_host", losses, states, initial_accel, K, R, best_states, best_accel, best_loss, best_index);
    if (rc != NGP_OK) return rc;
    const uint32_t best = ngp_select_best(losses, K);
    for (uint32_t e = 0; e < 4 * R; e++) best_states[e] = states[4 * (size_t)R * best + e];
    for (uint32_t e = 0; e < 2; e++) best_accel[e] = initial_accel[2 * (size_t)best + e];
    *best_loss = losses[best];
    *best_index = best;
    return NGP_OK;
}
