// The scalar LGSSM's Kalman message steps (lgssm/helper.py:53-192), shared by the exact-score unit (pfg_kalman.hip,
// PFG_SMOOTHER_KALMAN) and the forward-filtering backward-sampling unit (pfg_ffbs.hip, PFG_SMOOTHER_KALMAN_FFBS).
// The arithmetic follows the reference's NumPy expressions operation by operation: both units build with
// -ffp-contract=off and 1 x 1 solves are IEEE divisions.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct KalmanTheta {
    double A, C, LQinv, LRinv;
    double Qinv, Rinv, AtQinv, AtQinvA, CtRinv, CtRinvC, QinvA, RinvC;
};

struct Msg { double mp, P; };       // (mean_precision, precision)

__device__ __forceinline__ KalmanTheta kalman_theta(const double *th) {
    KalmanTheta k;
    k.A = th[0]; k.C = th[1]; k.LQinv = th[2]; k.LRinv = th[3];
    k.Qinv = k.LQinv * k.LQinv;
    k.Rinv = k.LRinv * k.LRinv;
    k.AtQinv = k.A * k.Qinv;
    k.AtQinvA = k.AtQinv * k.A;
    k.CtRinv = k.C * k.Rinv;
    k.CtRinvC = k.CtRinv * k.C;
    k.QinvA = k.Qinv * k.A;
    k.RinvC = k.Rinv * k.C;
    return k;
}

// one step of _forward_messages: the message of x_{t-1} and y_t -> the message of x_t; *log_c = log Pr(y_t | y_{<t})
__device__ __forceinline__ Msg kalman_forward(const KalmanTheta &k, Msg f, double y, double *log_c) {
    const double J = k.AtQinv / (k.AtQinvA + f.P);
    const double pred_mp = J * f.mp;
    const double pred_P = k.Qinv - k.AtQinv * J;
    const double y_mean = k.C * (pred_mp / pred_P);
    const double y_prec = k.Rinv - k.CtRinv * (k.CtRinv / (k.CtRinvC + pred_P));
    const double r = y - y_mean;
    *log_c = (-0.5 * (r * (y_prec * r)) + 0.5 * log(fabs(y_prec))) + -0.9189385332046727;   // -0.5 m log(2 pi), m = 1
    return Msg{pred_mp + k.CtRinv * y, pred_P + k.CtRinvC};
}

// one step of _backward_messages: the message of x_t and y_t -> the message of x_{t-1} (its log constant is not needed)
__device__ __forceinline__ Msg kalman_backward(const KalmanTheta &k, Msg b, double y) {
    const double xi = (k.Qinv + b.P) + k.CtRinvC;
    const double L = k.AtQinv / xi;
    const double vi = b.mp + k.CtRinv * y;
    return Msg{L * vi, k.AtQinvA - k.AtQinv * L};
}

}  // namespace
