"""ecgmm_signal_resample through ctypes, for tests/test_resample_ops_gpu.py: the output is a NaN-filled view between sentinel
zones (tests/tabnet_abi.call asserts that every element is written and nothing next to it), the workspace is NaN-filled,
exactly as large as the library asks and followed by sentinels, out_lengths lies between sentinel cells."""
import numpy as np
import torch

from ecgmm.hip import lib as L
from ecgmm.hip.functional import ptr

from .lstm_abi import DEV, guarded_bytes, tail_touched
from .tabnet_abi import call

LEN_GUARD = 64
LEN_SENTINEL = -777


def resample(x, num=0, ratio=0.0, lengths=None, T_out=None, out_lengths=False, expect=0):
    """x [S, L] (numpy or torch, fp32 values; NaN allowed behind a row's length).  Without lengths: L -> num.  With lengths
    (any ints): num = 0, T_out defaults to int(L * ratio).  -> out [S, T_out] float32 numpy (and int32 [S] out_lengths)."""
    x_ = torch.from_numpy(np.array(x, dtype=np.float32)).to(DEV).contiguous()
    S, Ln = x_.shape
    if T_out is None:
        T_out = int(Ln * ratio) if lengths is not None else num
    lib = L.lib()
    nb = lib.ecgmm_signal_resample_workspace(S, Ln, T_out)
    assert nb > 0 and nb % 16 == 0, lib.ecgmm_last_error()
    ws = guarded_bytes(nb)
    lens = None if lengths is None else torch.as_tensor(np.asarray(lengths, dtype=np.int32)).to(DEV)
    ol = torch.full((S + 2 * LEN_GUARD,), LEN_SENTINEL, dtype=torch.int32, device=DEV) if out_lengths else None
    r = call("ecgmm_signal_resample", {"out": (S, T_out)},
             lambda v: (ptr(x_), S, Ln, ptr(lens), num, ratio, ptr(v["out"]), T_out,
                        None if ol is None else ptr(ol[LEN_GUARD:]), ptr(ws), nb), expect=expect)
    assert not tail_touched(ws), "signal_resample wrote past its workspace"
    if ol is not None:
        assert bool((ol[:LEN_GUARD] == LEN_SENTINEL).all()) and bool((ol[-LEN_GUARD:] == LEN_SENTINEL).all()), \
            "written next to out_lengths"
    if expect:
        if ol is not None:
            assert bool((ol == LEN_SENTINEL).all()), "a refused call wrote out_lengths"
        return None
    out = r["out"].numpy()
    return (out, ol[LEN_GUARD:LEN_GUARD + S].cpu().numpy()) if out_lengths else out
