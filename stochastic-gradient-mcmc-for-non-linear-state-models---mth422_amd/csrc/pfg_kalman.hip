// Exact (Kalman) score and log-likelihood of the scalar LGSSM on buffered windows: PFG_SMOOTHER_KALMAN, the
// reference's kind = 'marginal' gradient (sgmcmc_sampler.py:298-329).  For one descriptor:
//   left buffer  [0, t1):  forward messages from the prior message of x_{-1}     (lgssm/helper.py:53-122)
//   right buffer [tL, T):  backward messages from the zero message               (:124-192)
//   window       [t1, tL): gradient_marginal_loglikelihood(include_init=True)    (:312-420)
//                          and the forward-only log-likelihood sum_t w_t log c_t (sgmcmc_sampler.py:147-174)
// out[0..3] = the gradient in LGSSM score column order [LRinv, LQinv, C, A], out[4] = the log-likelihood, out[5..7] = 0:
// the record the SGLD / SGHMC updates consume.  prior_mean / prior_var are the mean and variance of x_{-1}, i.e.
// mean_precision / precision and 1 / precision of the message.  An invalid descriptor gets out[0..7] = NaN.
//
// One lane per window, one wave per workgroup.  Per lane four sequential sweeps: backward over the right buffer and
// forward over the left one (last message kept), backward over the window storing every backward message
// b[t+1], t = 0..L-1, in the descriptor's scratch (16 L bytes; the ABI asks for 16 (L + 1) rounded up to 256), and
// forward over the window, which combines each forward message with the stored backward one.  Summing forward keeps
// the reference's order of every accumulation.  Built with -ffp-contract=off: the arithmetic follows the reference's
// NumPy expressions operation by operation (1 x 1 solves are divisions); the 2 x 2 joint precision of
// (x_{t-1}, x_t) is inverted through its cancellation-free determinant
//   det = P_f (P_b + C^2 Rinv + Qinv) + A^2 Qinv (P_b + C^2 Rinv).
#include "pfg_host.hpp"
#include "pfg_kalman.hpp"

namespace {

__global__ __launch_bounds__(64) void kalman_window_kernel(int B, const pfg_dev_problem *__restrict__ dp) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const pfg_dev_problem &d = dp[b];
    double *out = d.out;
    const int T = d.T, t1 = d.t1;
    const int tL = d.tL < T ? d.tL : T;
    const int L = tL - t1;
    const double prior_var = d.prior_var;
    const bool ok = out && d.theta && T >= 0 && t1 >= 0 && L >= 0 && (T == 0 || d.y) && (L == 0 || d.scratch) &&
                    prior_var > 0.0 && prior_var < INFINITY && isfinite(d.prior_mean);
    if (!ok) {
        if (out)
            for (int i = 0; i < PFG_OUT_DOUBLES; ++i) out[i] = NAN;
        return;
    }
    const KalmanTheta k = kalman_theta(d.theta);
    const double *__restrict__ y = d.y;
    const double *__restrict__ w = d.weights;
    double2 *__restrict__ bm = static_cast<double2 *>(d.scratch);

    // 1. right buffer, from the zero message: b[L], the message of x_{tL-1}
    Msg bk{0.0, 0.0};
    for (int t = T - 1; t >= tL; --t) bk = kalman_backward(k, bk, y[t]);
    // 2. left buffer, from the prior message of x_{-1}: f[0], the message of x_{t1-1}
    const double P0 = 1.0 / prior_var;
    Msg f{d.prior_mean * P0, P0};
    for (int t = 0; t < t1; ++t) {
        double lc;
        f = kalman_forward(k, f, y[t], &lc);
    }
    // 3. window, backward: bm[t] = b[t+1], the message of x_{t1+t} given y_{>t1+t}
    for (int t = L - 1; t >= 0; --t) {
        bm[t] = make_double2(bk.mp, bk.P);
        if (t > 0) bk = kalman_backward(k, bk, y[t1 + t]);
    }
    // 4. window, forward: transition term (f[t], b[t+1], y_t), filter step, emission term (f[t+1], b[t+1], y_t)
    const double LQinv_diaginv = 1.0 / k.LQinv, LRinv_diaginv = 1.0 / k.LRinv;
    double gA = 0.0, gC = 0.0, gLQ = 0.0, gLR = 0.0, ll = 0.0;
    for (int t = 0; t < L; ++t) {
        const double yt = y[t1 + t];
        const double wt = w ? w[t] : 1.0;
        const double2 bb = bm[t];
        {   // Pr(x_{t-1}, x_t | y): 2 x 2 precision [[a, c], [c, e]], c = -QinvA
            const double a = f.P + k.AtQinvA, c = -k.QinvA, e = (bb.y + k.CtRinvC) + k.Qinv;
            const double r1 = f.mp, r2 = bb.x + k.RinvC * yt;
            const double det = f.P * e + k.AtQinvA * (bb.y + k.CtRinvC);
            const double cov_pp = e / det, cov_np = -c / det, cov_nn = a / det;
            const double xp = (e * r1 - c * r2) / det, xn = (a * r2 - c * r1) / det;
            const double xpxp = cov_pp + xp * xp, xnxp = cov_np + xn * xp, xnxn = cov_nn + xn * xn;
            gA += wt * (k.Qinv * (xnxp - k.A * xpxp));
            const double Axpxn = k.A * xnxp, AxpxpA = k.A * (xpxp * k.A);
            gLQ += wt * (LQinv_diaginv + -1.0 * ((((xnxn - Axpxn) - Axpxn) + AxpxpA) * k.LQinv));
        }
        double lc;
        f = kalman_forward(k, f, yt, &lc);
        ll += lc * wt;
        {   // Pr(x_t | y)
            const double cmp = f.mp + bb.x, cP = f.P + bb.y;
            const double x = cmp / cP;
            const double xx = 1.0 / cP + x * x;
            gC += wt * ((k.Rinv * yt) * x + -1.0 * (k.RinvC * xx));
            const double Cxy = (k.C * x) * yt, CxxC = k.C * (xx * k.C);
            gLR += wt * (LRinv_diaginv + -1.0 * ((((yt * yt - Cxy) - Cxy) + CxxC) * k.LRinv));
        }
    }
    out[0] = gLR; out[1] = gLQ; out[2] = gC; out[3] = gA;
    out[4] = ll;
    out[5] = 0.0; out[6] = 0.0; out[7] = 0.0;
}

}  // namespace

namespace pfg_host {

int launch_kalman(pfg_ctx *ctx, const LaunchPlan &, int B, const pfg_dev_problem *dp, hipStream_t st) {
    if (B <= 0) return PFG_OK;
    hipLaunchKernelGGL(kalman_window_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, B, dp);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}

}  // namespace pfg_host
