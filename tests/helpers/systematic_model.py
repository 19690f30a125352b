"""Systematic resampling (PFG_SMOOTHER_NEMETH_SYSTEMATIC, resampling='systematic', variant systematic256x4) restated on the
pinned CPU oracle.

Child r of a timestep searches the unchanged CDF with u_r = (r + u0) / N, ONE u0 ~ U[0, 1) per step on the 32-bit grid
(w + 0.5) / 2^32, w the next word of lane 0's keyed generator.  The kernel computes (r + u0) * (1 / N) in fp64 and its
traced launch records the uniform every child searched with (rec_ud), so the offset, the generator word behind it and the
whole search are recovered from the record.  The reference has no systematic resampler: there is no REPLAY stream, and
what pins the resampler beside the replay is its defining property, checked by `offspring_violations` from the
log-weights and the ancestors alone."""
import numpy as np

from oracle import pf_oracle as po

SLOTS = 1024            # CDF slots of systematic256x4: index order, fp64 entries, the layout stratified256x4 shares


def systematic_uniforms(u0, N):
    """The N uniforms of one step, (r + u0) * (1 / N): one rounding of 1 / N and one of the product, as the kernel."""
    return (np.arange(N) + u0) * (1.0 / N)


def device_ancestors(logw, ud):
    """Ancestors as systematic256x4 lays the search out, from the uniforms a launch recorded: slot i <-> particle i, fp64
    entries cs / W over 1024 slots, slots >= N weighing nothing, against the uniform itself."""
    return po.device_ancestors(logw, ud, SLOTS, 1, "f64_uniform")


def offsets(ud):
    """ud [T, N] recorded uniforms -> (u0 [T], words [T] int64, dist [T]): child 0 searched with u0 / N, so u0_t =
    ud[t, 0] * N; the generator word behind it is w = u0 * 2^32 - 0.5, returned rounded with its distance from an integer."""
    ud = np.asarray(ud, dtype=np.float64)
    N = ud.shape[1]
    u0 = ud[:, 0] * N
    raw = u0 * 4294967296.0 - 0.5
    words = np.rint(raw)
    return u0, words.astype(np.int64), np.abs(raw - words)


def offspring_violations(anc, logw, delta):
    """The number of parents whose offspring count n_i lies outside [floor(N p_i - delta), ceil(N p_i + delta)], p =
    softmax(logw) in fp64: systematic resampling gives every parent floor(N p_i) or ceil(N p_i) children, whatever u0 is."""
    logw = np.asarray(logw, dtype=np.float64)
    N = logw.shape[0]
    p = np.exp(logw - np.max(logw))
    p /= p.sum()
    n = np.bincount(np.asarray(anc, dtype=np.int64), minlength=N)
    return int(np.sum((n < np.floor(N * p - delta)) | (n > np.ceil(N * p + delta))))


def in_order_subsequence(words, stream_words):
    """Whether `words` occur, in this order, in `stream_words` (other words may lie between them)."""
    it = iter([int(w) for w in stream_words])
    return all(any(int(w) == s for s in it) for w in words)
