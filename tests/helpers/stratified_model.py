"""Stratified resampling (PFG_SMOOTHER_NEMETH_STRATIFIED, resampling='stratified') restated on the pinned CPU oracle.

Child r of a timestep searches the unchanged CDF with u'_r = (r + U_r) / N, one U_r ~ U[0, 1) per child.  With the REPLAY
generator U_r is the stream's u[t][r], so the specification is `oracle.pf_oracle.pf_window` fed `stratified_uniforms(u)` in
place of u: NumPy's (np.arange(N) + u) / N is one fp64 addition and one IEEE division per child, which is what the REPLAY
kernels compute (include/pfgrad.h).  The DEVICE instantiations record the uniform every child searched with (rec_ud); their
CDF layouts are restated by `device_ancestors` below."""
import numpy as np

from oracle import pf_oracle as po

# CDF slots of the DEVICE instantiations, by variant name (pfg_last_variant)
SLOTS = {"stratified256x4": 1024, "big4096_stratified": 4096, "big16384_stratified": 16384}


def stratified_uniforms(u):
    """u [..., N] uniforms of a multinomial run -> the stratified ones, (r + u[..., r]) / N."""
    u = np.asarray(u, dtype=np.float64)
    N = u.shape[-1]
    return (np.arange(N) + u) / N


def pf_window(model, theta, y, N, z0, u, z, **kw):
    """po.pf_window with stratified resampling on the streams (z0, u, z) of a multinomial run."""
    return po.pf_window(model, theta, y, N, z0, stratified_uniforms(u), z, **kw)


def device_ancestors(logw, ud, variant):
    """Ancestors as the stratified DEVICE instantiations lay the search out, from the uniforms a launch recorded.  All
    three keep the CDF in PARTICLE order (slot i <-> particle i: the 256 x 4 instantiation is not the thread-major BLK
    layout of the multinomial unit; the large-N twin is pf_big_kernel's), fp64 entries cs / W over `SLOTS[variant]`
    slots, slots >= N weighing nothing, against the uniform itself: po.device_ancestors with one particle per "thread"."""
    return po.device_ancestors(logw, ud, SLOTS[variant], 1, "f64_uniform")


def run_windows(problems, ctx=None, want_final=False):
    """Stand-in for particle_filters.run_windows on the CPU: tests/oracle_backend.run_windows_oracle, with windows of the
    'nemeth_stratified' smoother mapped onto NEMETH windows with the transformed uniforms."""
    from oracle_backend import run_windows_oracle
    mapped = []
    for q in problems:
        if q["smoother"] == "nemeth_stratified":
            q = dict(q, smoother="nemeth", u=stratified_uniforms(q["u"]))
        mapped.append(q)
    return run_windows_oracle(mapped, ctx, want_final)
