"""Window descriptors a device sampler wrote (pfg_dev_problem records) read back as host windows."""
import numpy as np


def decode(desc, y_ptr, weights_ptr=0):
    """desc: the descriptors (a device tensor or bytes-like) -> (records, y offset, weights offset or -1), offsets in
    doubles from y_ptr / weights_ptr."""
    from sgmcmc_ssm_amd import _capi
    raw = desc.cpu().numpy() if hasattr(desc, "cpu") else np.asarray(desc)
    d = raw.reshape(-1).view(np.uint8).view(_capi.DEV_PROBLEM_DTYPE)
    yoff = (d["y"].astype(np.int64) - int(y_ptr)) // 8
    woff = np.where(d["weights"] == 0, -1, (d["weights"].astype(np.int64) - int(weights_ptr or 0)) // 8)
    return d, yoff, woff


def ensemble_windows(ens):
    """The device-written descriptors of the latest step of a ChainEnsemble: [C*W] records, y offsets, weights offsets
    (or -1) and the sequence lengths."""
    d, yoff, woff = decode(ens.desc_dev, ens.y_dev.data_ptr(),
                           ens.weights_dev.data_ptr() if ens.weights_dev is not None else 0)
    _, seq_len = ens.window_statistics()
    return d, yoff, woff, seq_len.reshape(-1)
