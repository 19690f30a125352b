"""NumPy restatement of pfg_reduce_windows_device (include/pfgrad.h): the W = K * M window records of one chain ->
one record, in the reference's order of operations (sgmcmc_sampler.py:411-418 within a sequence, :1264-1282 across
sequences and the T_total / S rescaling).  Shared by the CPU pin against the drop-in and the GPU tests."""
import numpy as np

COLS = 5        # out[0..3] score columns, out[4] log-likelihood


def reduce_chain(records, seq_len, K, M, rescale, T_total):
    """records [K*M, 8], seq_len [K*M] -> [8] (out[5..7] = 0)."""
    acc = None
    S = 0.0
    for k in range(K):
        part = np.zeros(COLS)
        for m in range(M):
            g = np.asarray(records[k * M + m][:COLS], dtype=np.float64)
            part = part + g * 1.0 / M
        acc = part if acc is None else acc + part
        S += int(seq_len[k * M])
    if rescale:
        acc = acc * float(T_total) / S
    out = np.zeros(8)
    out[:COLS] = acc
    return out


def reduce_windows(records, seq_len, K, M, rescale, T_total):
    """records [C, W, 8] (or [C*W, 8]), seq_len [C, W] -> [C, 8]."""
    W = K * M
    records = np.asarray(records).reshape(-1, W, 8)
    seq_len = np.asarray(seq_len).reshape(-1, W)
    return np.stack([reduce_chain(r, s, K, M, rescale, T_total) for r, s in zip(records, seq_len)])
