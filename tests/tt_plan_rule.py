"""NumPy restatement of what ``pcx_tt_create`` decides about a tensor train (csrc/tt_plan.h): the validation, the four
evaluation forms beside the generic one and their geometry, the LDS of each launch, which form a launch takes, and the
layouts of the host-built core images.  Written from the rules as the handle has always applied them, not from the
planner's code; tests/test_tt_plan_host.py holds the planner to it field for field.  No GPU.

A plan is a dict keyed as tests/host/tt_plan_main.cpp prints it.  Cores are G_k[a][j][b], concatenated."""
from __future__ import annotations

import numpy as np

INVALID, UNSUPPORTED = -1, -4
MAX_DIMS = 16
KIB = 1024
NO_WFIRST = "W-first TT kernel does not cover this model"
NO_D4 = "4x4x4 direct TT kernel does not cover this model"
NO_LPP = "lane-per-point TT kernel does not cover this model"
GENERIC_ONLY = "ranks above 64 run on the generic kernel only"


def _ceil(a: int, b: int) -> int:
    return -(-a // b)


def cores(seed: int, total: int) -> np.ndarray:
    """core[i] = splitmix64(seed + i + 1) / 2^64 - 1/2, the top 53 bits of the hash"""
    with np.errstate(over="ignore"):
        x = np.uint64(seed) + np.arange(1, total + 1, dtype=np.uint64)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5


def plan(d, n, ranks, lo, hi, order):
    """{"rc", "error"} of a model that is refused, else {"rc": 0, "plan": {...}}.  Any of the arrays may be None (a missing
    array; a missing ``order`` is the identity)."""
    def refuse(code, text):
        return {"rc": code, "error": text}

    if d < 1 or d > MAX_DIMS:
        return refuse(INVALID, f"d={d} outside [1, {MAX_DIMS}]")
    if n is None or ranks is None or lo is None or hi is None:
        return refuse(INVALID, "NULL model array")
    if ranks[0] != 1 or ranks[d] != 1:
        return refuse(INVALID, "boundary TT ranks must be 1")
    seen = set()
    col = []
    for k in range(d):
        if not 1 <= n[k] <= 4096 or ranks[k] < 1 or ranks[k + 1] < 1:
            return refuse(INVALID, f"bad n_nodes/ranks at dim {k}")
        if not lo[k] < hi[k]:
            return refuse(INVALID, f"domain[{k}]: lo must be < hi")
        c = k if order is None else order[k]
        if not 0 <= c < d or c in seen:
            return refuse(INVALID, "dim_order is not a permutation")
        seen.add(c)
        col.append(c)
    n, ranks = [int(v) for v in n[:d]], [int(v) for v in ranks[:d + 1]]
    rmax, nmax = max(ranks), max(n)
    sizes = [ranks[k] * n[k] * ranks[k + 1] for k in range(d)]
    coff = [sum(sizes[:k]) for k in range(d)]
    zeros = [0] * d
    p = {"d": d, "n": n, "col": col, "lo": [float(v) for v in lo[:d]], "hi": [float(v) for v in hi[:d]],
         "scale": [2.0 / (float(hi[k]) - float(lo[k])) for k in range(d)], "frag_off": zeros, "ranks": ranks, "coff": coff,
         "core_total": sum(sizes), "frag_total": 0, "rmax": rmax, "nmax": nmax, "generic": 0,
         "gi.rank": [0] * (d + 1), "gi.coff": zeros, "gi.rmax": 0, "gi.nmax": 0,
         "cls": 0, "rk.rc": zeros, "rk.rt": zeros, "rl_last": 0, "last_rows": 0, "last_lds_doubles": 0,
         "wR": 0, "wplan.ntiles": zeros, "wplan.lds_off": zeros, "wplan.ks": 0, "wplan.total": 0,
         "d4RA": 0, "d4plan.lds_off": zeros, "d4plan.total": 0, "d4_preferred": 1,
         "lppCap": 0, "lpp_nodes": 0, "lpp_preferred": 0}
    if rmax > 64:
        if rmax > 4096:
            return refuse(UNSUPPORTED, f"TT rank {rmax} > 4096")
        if 4 * (2 * rmax + nmax) * 8 > 160 * KIB:
            return refuse(UNSUPPORTED, f"TT rank {rmax} with {nmax} nodes exceeds the generic kernel's LDS budget "
                                       "(2 rank + nodes <= 5120)")
        p.update({"generic": 1, "gi.rank": ranks, "gi.coff": coff, "gi.rmax": rmax, "gi.nmax": nmax})
        return {"rc": 0, "plan": p}

    # the 16x16x4 direct form: every model with ranks <= 64 has it
    cls = 0 if rmax <= 16 else (1 if rmax <= 32 else 2)
    RC = (_ceil(rmax, 4), 8, 16)[cls]
    RT = (1, 2, 4)[cls]
    rc = [1] + [RC] * (d - 1)
    blocks = [n[k] * rc[k] * RT * 64 for k in range(d)]
    last = 4 * RC * n[-1]
    p.update({"cls": cls, "rk.rc": rc, "rk.rt": [RT] * d, "frag_off": [sum(blocks[:k]) for k in range(d)],
              "frag_total": sum(blocks), "rl_last": ranks[d - 1], "last_rows": 4 * RC,
              "last_lds_doubles": last if last * 8 <= 16 * KIB else 0})

    # W-first: the geometry whenever the ranks and node counts allow it, the form itself inside 96 KiB
    if rmax <= 12 and nmax <= 32:
        R, ks = 4 * _ceil(rmax, 4), _ceil(nmax, 4)
        ntiles = [_ceil(R, 16)] + [R * R // 16] * (d - 1)
        blocks = [ks * ntiles[k] * 64 for k in range(d - 1)] + [R * 4 * ks]
        p.update({"wplan.ntiles": ntiles, "wplan.lds_off": [sum(blocks[:k]) for k in range(d)], "wplan.ks": ks,
                  "wplan.total": sum(blocks), "wR": R if sum(blocks) * 8 <= 96 * KIB else 0})

    # 4x4x4: likewise, inside 72 KiB of image, bounds table and per-wave query rows and records
    if rmax <= 12 and nmax <= 16:
        RA = _ceil(rmax, 4)
        NMP = 4 if RA == 3 else RA
        blocks = [(_ceil(n[k], 4) * 16 * NMP if k == 0 else n[k] * RA * 16 * NMP) for k in range(d - 1)] + [4 * RA * n[-1]]
        p.update({"d4plan.lds_off": [sum(blocks[:k]) for k in range(d)], "d4plan.total": sum(blocks)})
        if (sum(blocks) + 2 * 16 * d + 4 * (16 * d + 96)) * 8 <= 72 * KIB:
            p["d4RA"] = RA
            if p["wR"] and RA > 1:
                c4 = sum(n[k] * RA * RA * 20 + 100 for k in range(1, d - 1))
                cw = sum((p["wR"] ** 2 // 16) * p["wplan.ks"] * 75 + 160 for k in range(1, d - 1))
                p["d4_preferred"] = int(c4 <= cw)

    if rmax <= 16 and nmax <= 16:
        p.update({"lppCap": 8 if rmax <= 8 else (12 if rmax <= 12 else 16), "lpp_nodes": n[0] if len(set(n)) == 1 else 0,
                  "lpp_preferred": int(rmax <= 15)})
    return {"rc": 0, "plan": p}


def lds(p):
    """dynamic LDS bytes per launch, keyed as the program prints them (W-first at NT = 1, 4; direct at nt = 1, 2, 4)"""
    d = p["d"]
    return {"generic": 4 * (2 * p["rmax"] + p["nmax"]) * 8,
            "d4": (p["d4plan.total"] + 2 * 16 * d + 4 * (16 * d + 96)) * 8,
            "wfirst": [(p["wplan.total"] + 6 * 16 * nt * d) * 8 for nt in (1, 4)],
            "direct": [(4 * 16 * nt * d + p["last_lds_doubles"]) * 8 for nt in (1, 2, 4)],
            "lpp": p["rmax"] * 64 * 8}


def auto_variant(p, requested, wfirst=True, d4=True, lpp=True):
    """The form a launch takes (0 generic, 1 16x16x4, 2 W-first, 3 4x4x4, 4 lane per point) or the refusal's text;
    wfirst / d4 / lpp: the image was uploaded."""
    w, d4, lpp = bool(p["wR"]) and wfirst, bool(p["d4RA"]) and d4, bool(p["lppCap"]) and lpp
    for variant, there, text in ((2, w, NO_WFIRST), (3, d4, NO_D4), (4, lpp, NO_LPP)):
        if requested == variant:
            return variant if there else text
    if p["generic"]:
        return GENERIC_ONLY if requested else 0
    if requested == 1:
        return 1
    if lpp and p["lpp_preferred"]:
        return 4
    if d4 and (not w or p["d4_preferred"]):
        return 3
    return 2 if w else 1


def _G(p, c, k):
    return c[p["coff"][k]:][:p["ranks"][k] * p["n"][k] * p["ranks"][k + 1]].reshape(p["ranks"][k], p["n"][k], p["ranks"][k + 1])


def last_core(p, c):
    """[last_rows][n] : the last core's [a][j], zero rows behind its rank"""
    out = np.zeros((p["last_rows"], p["n"][-1]))
    out[:p["ranks"][-2]] = _G(p, c, p["d"] - 1)[:, :, 0]
    return out.ravel()


def d4_image(p, c):
    """dim 0: [s][slot = 4 k + i][NMP] = G_0[0][4 s + k][4 m + i]; mid dims: [j][c][slot][NMP] = G_k[4 c + k][j][4 m + i];
    last dim: [4 RA][n] = G[a][j][0]; zero past the true ranks and nodes (and in the NMP - RA padding of a slot)"""
    d, RA = p["d"], p["d4RA"]
    NMP = 4 if RA == 3 else RA
    img = np.zeros(p["d4plan.total"])
    for k in range(d):
        G = _G(p, c, k)
        rl, nk, rr = G.shape
        off = p["d4plan.lds_off"][k]
        if k == d - 1:
            blk = np.zeros((4 * RA, nk))
            blk[:rl] = G[:, :, 0]
        elif k == 0:
            pad = np.zeros((4 * _ceil(nk, 4), 4 * RA))
            pad[:nk, :rr] = G[0]
            blk = np.zeros((_ceil(nk, 4), 4, 4, NMP))                                     # [s][k][i][m]
            blk[..., :RA] = pad.reshape(-1, 4, RA, 4).transpose(0, 1, 3, 2)              # [s][k][m][i] -> [s][k][i][m]
        else:
            pad = np.zeros((4 * RA, nk, 4 * RA))
            pad[:rl, :, :rr] = G
            blk = np.zeros((nk, RA, 4, 4, NMP))                                           # [j][c][k][i][m]
            blk[..., :RA] = pad.reshape(RA, 4, nk, RA, 4).transpose(2, 0, 1, 4, 3)       # [c][k][j][m][i] -> [j][c][k][i][m]
        img[off:off + blk.size] = blk.ravel()
    return img


def lpp_image(p, c):
    """img[off_k + (b rl + a) n + j] = G_k[a][j][b], 64 zeros behind the end"""
    return np.concatenate([_G(p, c, k).transpose(2, 0, 1).ravel() for k in range(p["d"])] + [np.zeros(64)])


def lpp_table(p):
    """per storage dimension [off, rl, rr, n, col, 0, lo, scale]"""
    return [[p["coff"][k], p["ranks"][k], p["ranks"][k + 1], p["n"][k], p["col"][k], 0, p["lo"][k], p["scale"][k]]
            for k in range(p["d"])]
