"""Shared by tests/test_gpu_dp.py and tests/enum_mode_cases.py: the inputs of the two tabulated gap models
(ALN_GAP_DEL_TABLE_INS_TPOS, ALN_GAP_TABLES), built on the host from numpy and the oracle's gap functions.  Nothing here
imports the HIP library."""
import ctypes as C

import numpy as np

import orc


def gn2_tables(rng, T):
    """Synthetic Gn2Eval::pre_calculate outputs (gn2_eval.cpp:113-158) for a template of T positions: v_gi/v_ge/v_cn and the
    (p2,p1)-indexed distance / vv_gi / vv_ge / vv_cd tables.  Real inputs come from the Troll library (absent)."""
    t = {"v_gi": rng.uniform(3, 9, T), "v_ge": rng.uniform(0.1, 0.9, T), "v_cn": rng.uniform(-0.5, 1.5, T),
         "dist": rng.uniform(3, 30, (T, T)), "vv_gi": rng.choice([4.0, 9.5], (T, T)), "vv_ge": rng.choice([0.2, 0.7], (T, T)),
         "vv_cd": np.exp(rng.uniform(-6, 1, (T, T)))}
    return {k: v.astype(np.float32) for k, v in t.items()}


def gn2_deletion_table(tb, T, mode):
    """What a host lowering of Gn2Eval materialises: deletion(t1,t2) for every t1 < t2 (gn2_eval.h:100-130), fp32."""
    D = np.zeros((T, T), dtype=np.float32)
    for t1 in range(T):
        for t2 in range(t1 + 2, T):
            p1, p2 = t1, t2 - 2
            gp = np.float32(8100.0)
            if tb["dist"][p2, p1] < np.float32(18.0):
                gp = np.float32(np.float32(tb["vv_gi"][p2, p1] + np.float32(tb["vv_ge"][p2, p1] * np.float32(t2 - t1 - 2))) + tb["vv_cd"][p2, p1])
            if mode in (3, 4, 2) and (t1 == 0 or t2 == T - 1):
                gp = np.float32(0.0)
            D[t1, t2] = gp
    return D


def tabulate_gaps(gap, Q, T):
    """What aln_lowering.h does for an arbitrary evaluator, here with the oracle's gap functions as "the evaluator":
    deletion(t1,t2) for every t1 < t2, insertion for interior / head / tail query positions."""
    L = orc.lib()
    err = C.c_int(0)
    D = np.zeros((T, T), dtype=np.float32)
    for t1 in range(T):
        for t2 in range(t1 + 1, T):
            D[t1, t2] = L.orc_deletion(gap.ref, Q, T, 1, 2, t1, t2, C.byref(err))
    I = np.zeros((3, T, Q), dtype=np.float32)
    for t1 in range(T - 1):
        for d in range(1, Q - 2):
            I[0, t1, d] = L.orc_insertion(gap.ref, Q, T, 1, 1 + d, t1, t1 + 1, C.byref(err))
        for q2 in range(1, Q):
            I[1, t1, q2] = L.orc_insertion(gap.ref, Q, T, 0, q2, t1, t1 + 1, C.byref(err))
        for q1 in range(0, Q - 1):
            I[2, t1, q1] = L.orc_insertion(gap.ref, Q, T, q1, Q - 1, t1, t1 + 1, C.byref(err))
    assert err.value == 0
    return D, I
