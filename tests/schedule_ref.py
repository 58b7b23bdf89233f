"""The contract of vsom_batch_schedule (include/vsom_hip.h) restated as the loop of single epochs it stands for:

    for ep in 0 .. epochs-1:
        if ep > 0 and reset_bmu: lastBMU := 0            (the reference's per-epoch reload, DataSet.cpp:136-137)
        batch_epoch(sigma[ep], ep == 0)

oracle_loop runs it on the CPU oracle, twin_loop on a device context through the single-epoch call."""
import numpy as np


def oracle_loop(o, X, sigmas, reset_bmu=True):
    """OracleSom `o` trained through the schedule on the one chunk X: (per-epoch MSE [float32], lastBMU [uint64])"""
    lb = np.zeros(X.shape[0], np.uint64)
    mse = np.zeros(len(sigmas), np.float32)
    for ep, sigma in enumerate(sigmas):
        if ep > 0 and reset_bmu:
            lb[:] = 0
        mse[ep] = o.batch_epoch(X, lb, sigma, ep == 0)
    return mse, lb


def twin_loop(ctx, sigmas, reset_bmu=True):
    """the same on a vsom_amd Context whose chunk is loaded: the per-epoch MSE [float32]"""
    zeros = np.zeros(ctx.chunk_size, np.uint64)
    mse = np.zeros(len(sigmas), np.float32)
    for ep, sigma in enumerate(sigmas):
        if ep > 0 and reset_bmu:
            ctx.set_last_bmu(zeros)
        mse[ep] = ctx.batch_epoch(sigma, ep == 0)
    return mse


def beq(a, b):
    """bitwise equality; NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())
