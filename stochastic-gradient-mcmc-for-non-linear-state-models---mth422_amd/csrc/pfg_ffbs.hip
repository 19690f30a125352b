// Forward-filtering backward-sampling (FFBS) of the scalar LGSSM's latent path on buffered windows:
// PFG_SMOOTHER_KALMAN_FFBS, the reference's LGSSMHelper.latent_var_sample(distr = 'joint') (lgssm/helper.py:650-698)
// and, on the sampled paths, the complete-data score of kind = 'complete' (sgmcmc_sampler.py:330-362,
// lgssm/helper.py:422-491).  For one descriptor, the buffer [0, T):
//   forward   once per window (lane 0): the Kalman messages (mp_t, P_t) of x_t given y_{<=t} from the message of x_{-1}
//             (prior_mean = mean_precision / precision, prior_var = 1 / precision, as for PFG_SMOOTHER_KALMAN), with
//             the arithmetic of kalman_forward (pfg_kalman.hpp).  The scratch keeps (mp_t, c_t) per step, where
//             c_{T-1} = 1 / P_{T-1} and c_t = 1 / (P_t + AtQinvA) below: 16 T bytes of kalman_scratch_bytes(T).
//   backward  one lane per path (lanes loop when N exceeds the workgroup), in the reference's operation order:
//               x_{T-1} = z sqrt(c_{T-1}) + c_{T-1} mp_{T-1}
//               x_t     = c_t (mp_t + AtQinv x_{t+1}) + (z sqrt(c_t) + 0.0)
//             (np.random.multivariate_normal of a 1 x 1 covariance is mean + z sqrt(cov)).  The normals: REPLAY
//             z[k N + s] is path s at time T-1-k (one np.random.standard_normal(T N) call); DEVICE the keyed lane
//             generator of the particle filters, lane = path, keyed by (seed, stream, *step_ctr).
//   score     stat = SCORE: the complete-data score over [t1, tL) averaged over the N paths, in the LGSSM score column
//             order [LRinv, LQinv, C, A], out[4..7] = 0.  Per time step, weight w_t, mean <.> over the paths:
//               A      w Qinv <(x_t - A x_{t-1}) x_{t-1}>     LQinv  w (1/LQinv - <(x_t - A x_{t-1})^2> LQinv)
//               C      w Rinv <(y_t - C x_t) x_t>             LRinv  w (1/LRinv - <(y_t - C x_t)^2> LRinv)
//             the two transition terms only where x_{t-1} is inside the buffer (t >= 1).  Each lane sums its paths'
//             terms, one workgroup reduction ends the window.  stat = NONE samples only (out[0..7] = 0).
//   gibbs     stat = GIBBS (N = 1 path): the sufficient statistics of LGSSMHelper.calc_gibbs_sufficient_statistic
//             (lgssm/helper.py:502-555) of the whole buffer's path, summed by its lane while it samples backward;
//             t1, tL and the weights are ignored.  out = [sum_{t>=1} x_{t-1}^2, sum_{t>=1} x_t x_{t-1},
//             sum_{t>=1} x_t^2, sum_t x_t^2, sum_t y_t x_t, sum_t y_t^2, T, 0]: what gibbs_update_kernel
//             (pfg_chains.hip) draws the parameters from.
//   paths     trace_x, when non-NULL: the sampled paths [T][N], t ascending.  Without it a SCORE window stops
//             sampling at t = t1 - 1.
// An invalid descriptor gets out[0..7] = NaN.  Built with -ffp-contract=off; IEEE division and ::sqrt throughout.
#include "pfg_host.hpp"
#include "pfg_kalman.hpp"
#include "pfg_math.hpp"

namespace {

// PFG_STAT_GIBBS: the one path of the buffer, sampled backward with the normals and arithmetic of the score loop below
// (same path), and the sufficient statistics of lgssm/helper.py:502-555 summed on the way
template <bool DEVICE>
__device__ __forceinline__ void ffbs_gibbs_path(const pfg_dev_problem &d, const KalmanTheta &k, const double2 *__restrict__ fm,
                                             double *__restrict__ trace, double *__restrict__ out) {
    const int T = d.T;
    const double *__restrict__ y = d.y;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (T > 0) {
        const pfg::Math<double, true> mth{};
        pfg::LaneRng g{};
        if (DEVICE) g = pfg::lane_rng_init(d.seed, d.stream, d.step_ctr ? *d.step_ctr : 0, 0u);
        double z_next = 0.0;
        bool have = false;
        auto normal = [&](int t) -> double {        // REPLAY: z[T-1-t]; DEVICE: Box-Muller pairs, as the score loop
            if (!DEVICE) return d.z[T - 1 - t];
            if (have) { have = false; return z_next; }
            const uint32_t a = g.next();
            const uint32_t b = g.next();
            double z0, z1;
            mth.normal_pair(a, b, z0, z1);
            z_next = z1; have = true;
            return z0;
        };
        const double2 mT = fm[T - 1];
        double x = normal(T - 1) * ::sqrt(mT.y) + mT.y * mT.x;
        if (trace) trace[T - 1] = x;
        s[3] += x * x;
        s[4] += y[T - 1] * x;
        for (int t = T - 2; t >= 0; --t) {
            const double2 m = fm[t];
            const double xp = m.y * (m.x + k.AtQinv * x) + (normal(t) * ::sqrt(m.y) + 0.0);
            if (trace) trace[t] = xp;
            s[0] += xp * xp;            // the transition of time t + 1
            s[1] += x * xp;
            s[2] += x * x;
            s[3] += xp * xp;            // the emission of time t
            s[4] += y[t] * xp;
            x = xp;
        }
        for (int t = T - 1; t >= 0; --t) s[5] += y[t] * y[t];
    }
    for (int i = 0; i < 6; ++i) out[i] = s[i];
    out[6] = (double)T;
    out[7] = 0.0;
}

template <int NT, bool DEVICE>
__global__ __launch_bounds__(NT) void ffbs_window_kernel(const pfg_dev_problem *__restrict__ dp) {
    const pfg_dev_problem &d = dp[blockIdx.x];
    const int tid = threadIdx.x;
    double *out = d.out;
    const int T = d.T, t1 = d.t1, N = d.N;
    const int tL = d.tL < T ? d.tL : T;
    const double prior_var = d.prior_var;
    const bool score = d.stat == PFG_STAT_SCORE;
    const bool gibbs = d.stat == PFG_STAT_GIBBS;
    const bool ok = out && d.theta && T >= 0 && N >= 1 && t1 >= 0 && t1 <= tL &&
                    (T == 0 || (d.y && d.scratch && (DEVICE || d.z))) &&
                    (score || d.stat == PFG_STAT_NONE || (gibbs && N == 1)) &&
                    prior_var > 0.0 && prior_var < INFINITY && isfinite(d.prior_mean);
    if (!ok) {
        if (out && tid == 0)
            for (int i = 0; i < PFG_OUT_DOUBLES; ++i) out[i] = NAN;
        return;
    }
    const KalmanTheta k = kalman_theta(d.theta);
    const double *__restrict__ y = d.y;
    const double *__restrict__ w = d.weights;
    double2 *__restrict__ fm = static_cast<double2 *>(d.scratch);

    // 1. forward messages of the whole buffer, once per window
    if (tid == 0 && T > 0) {
        const double P0 = 1.0 / prior_var;
        Msg f{d.prior_mean * P0, P0};
#pragma unroll 8
        for (int t = 0; t < T; ++t) {
            double lc;
            f = kalman_forward(k, f, y[t], &lc);
            fm[t] = make_double2(f.mp, t == T - 1 ? 1.0 / f.P : 1.0 / (f.P + k.AtQinvA));
        }
    }
    __syncthreads();

    // 2. backward sampling, one lane per path
    double *__restrict__ trace = d.trace_x;
    if (gibbs) {        // one path, lane 0's; its own loop keeps the score loop's registers as they are
        if (tid == 0) ffbs_gibbs_path<DEVICE>(d, k, fm, trace, out);
        return;
    }
    const int t_stop = (trace || !score || t1 == 0) ? 0 : t1 - 1;
    const uint64_t step = d.step_ctr ? *d.step_ctr : 0;
    const pfg::Math<double, true> mth{};
    double sA = 0.0, sQ = 0.0, sC = 0.0, sR = 0.0;
    for (int s = tid; s < N && T > 0; s += NT) {
        pfg::LaneRng g{};
        if (DEVICE) g = pfg::lane_rng_init(d.seed, d.stream, step, (uint32_t)s);
        double z_next = 0.0;
        bool have = false;
        auto device_normal = [&]() -> double {        // Box-Muller pairs, the second variate kept for the next step
            if (have) { have = false; return z_next; }
            const uint32_t a = g.next();
            const uint32_t b = g.next();
            double z0, z1;
            mth.normal_pair(a, b, z0, z1);
            z_next = z1; have = true;
            return z0;
        };
        const double *__restrict__ zs = DEVICE ? nullptr : d.z + s;      // zs[k N]: time T-1-k
        auto emission = [&](int t, double x) {
            if (!score || t < t1 || t >= tL) return;
            const double wt = w ? w[t - t1] : 1.0;
            const double diff = y[t] - k.C * x;
            sC += wt * (diff * x);
            sR += wt * (diff * diff);
        };
        const double2 mT = fm[T - 1];
        double x = (DEVICE ? device_normal() : zs[0]) * ::sqrt(mT.y) + mT.y * mT.x;
        if (trace) trace[(size_t)(T - 1) * N + s] = x;
        emission(T - 1, x);
        // blocks of U steps: the block's messages and REPLAY normals are loaded together, then the dependent chain runs
        constexpr int U = 8;
        for (int t = T - 2; t >= t_stop;) {
            const int n = t - t_stop + 1 < U ? t - t_stop + 1 : U;
            double2 mb[U];
            double zb[U];
#pragma unroll
            for (int j = 0; j < U; ++j)
                if (j < n) {
                    mb[j] = fm[t - j];
                    zb[j] = DEVICE ? 0.0 : zs[(size_t)(T - 1 - (t - j)) * N];
                }
#pragma unroll
            for (int j = 0; j < U; ++j)
                if (j < n) {
                    const int tj = t - j;
                    const double z = DEVICE ? device_normal() : zb[j];
                    const double xp = mb[j].y * (mb[j].x + k.AtQinv * x) + (z * ::sqrt(mb[j].y) + 0.0);
                    if (trace) trace[(size_t)tj * N + s] = xp;
                    if (score && tj + 1 >= t1 && tj + 1 < tL) {      // the transition term of time tj + 1
                        const double wt = w ? w[tj + 1 - t1] : 1.0;
                        const double diff = x - k.A * xp;
                        sA += wt * (diff * xp);
                        sQ += wt * (diff * diff);
                    }
                    emission(tj, xp);
                    x = xp;
                }
            t -= n;
        }
    }

    // 3. the mean over the paths: wave sums, then the waves in order (the same for a window alone or in a batch)
    __shared__ double red[4][NT / 64];
    const double v[4] = {pfg::wave_sum(sA), pfg::wave_sum(sQ), pfg::wave_sum(sC), pfg::wave_sum(sR)};
    if ((tid & 63) == 0)
        for (int j = 0; j < 4; ++j) red[j][tid >> 6] = v[j];
    __syncthreads();
    if (tid != 0) return;
    double tot[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < 4; ++j)
        for (int q = 0; q < NT / 64; ++q) tot[j] += red[j][q];
    double gA = 0.0, gLQ = 0.0, gC = 0.0, gLR = 0.0;
    if (score && T > 0) {
        double Wtr = 0.0, Wem = 0.0;        // the weights of the window's transition / emission terms
        for (int t = t1; t < tL; ++t) {
            const double wt = w ? w[t - t1] : 1.0;
            Wem += wt;
            if (t >= 1) Wtr += wt;
        }
        const double invN = 1.0 / (double)N;
        gA = k.Qinv * (tot[0] * invN);
        gLQ = Wtr * (1.0 / k.LQinv) - (tot[1] * invN) * k.LQinv;
        gC = k.Rinv * (tot[2] * invN);
        gLR = Wem * (1.0 / k.LRinv) - (tot[3] * invN) * k.LRinv;
    }
    out[0] = gLR; out[1] = gLQ; out[2] = gC; out[3] = gA;
    out[4] = 0.0; out[5] = 0.0; out[6] = 0.0; out[7] = 0.0;
}

template <int NT>
void launch_nt(int rng, int B, const pfg_dev_problem *dp, hipStream_t st) {
    if (rng == PFG_RNG_DEVICE)
        hipLaunchKernelGGL((ffbs_window_kernel<NT, true>), dim3((unsigned)B), dim3(NT), 0, st, dp);
    else
        hipLaunchKernelGGL((ffbs_window_kernel<NT, false>), dim3((unsigned)B), dim3(NT), 0, st, dp);
}

}  // namespace

namespace pfg_host {

int launch_ffbs(pfg_ctx *ctx, const LaunchPlan &p, int rng, int B, const pfg_dev_problem *dp, hipStream_t st) {
    if (B <= 0) return PFG_OK;
    if (p.nt == 64) launch_nt<64>(rng, B, dp, st);
    else if (p.nt == 128) launch_nt<128>(rng, B, dp, st);
    else launch_nt<256>(rng, B, dp, st);
    PFG_HIP(ctx, hipGetLastError());
    return PFG_OK;
}

}  // namespace pfg_host
