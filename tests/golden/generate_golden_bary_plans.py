"""Launch-plan signatures and output digests of the barycentric handle, one case per decision branch of handle creation.

    python tests/golden/generate_golden_bary_plans.py [--out tests/golden/g27_bary_plans.npz]

needs an MI355X and talks to the library through its C ABI only (pychebyshev_amd._lib).  For every case it creates a
handle on a seeded random tensor over Chebyshev nodes on [-1, 1] and records

  * the return code and error text of a create that fails, or
  * kernel_info[0..5], grid_info[0..3], tail_info[1..3] ([0], [4], [5] depend on the device and on the latest launch),
    which of set_kernel(2..5) are accepted,
  * up to 2^20 elements: the SHA-256 of eval_multi_batch at N = 200 seeded in-domain points (one full 128-point block and
    a ragged one) for the specs value, first order along dimension 0, first order along the last dimension -- on the
    kernel auto picks ("digest") and, where auto picks another one, on the MFMA kernel ("digest_mfma"),
  * cases marked `big`: the same at N = 65,536 + 200 for value, delta and gamma along dimension 0 (dim-0 groups, tail
    split) with count_gemms of that spec set,
  * cases marked `rot`: per dimension q, count_gemms of value plus the first order along q at that N -- 1 where the
    pair shares a GEMM (q > 0: on the rotated sub-model), 2 where it does not.

Every digest is evaluated twice; a case whose two runs differ is not written (its name is printed).  Switches the
library reads once per process (PCX_BARY_SQ) get a child process of their own; the per-handle ones share a second child.
tests/test_gpu_bary_plan.py measures the same records with the library under test and compares them field for field;
tests/test_bary_plan_host.py compares the signatures with the planner on a CPU.

The file written holds one JSON text ("records") and nothing else.
"""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "g27_bary_plans.npz")
N_SMALL = 200
N_BIG = 65536 + 200
DIGEST_MAX_ELEMS = 1 << 20


def _c(shape, env=None, **flags):
    return {"shape": list(shape), "env": dict(env or {}), **flags}


CASES = (
    # rows only
    [_c(s) for s in [(300,), (4096,)]]
    # no kernel: create fails UNSUPPORTED
    + [_c((4096, 4096))]
    # lane-per-point preferred / available
    + [_c(s) for s in [(8, 8), (20, 64), (48, 64), (50, 50), (16, 16, 16), (8, 8, 50)]]
    # k_bary_sq rules
    + [_c(s) for s in [(12, 12), (6,) * 4, (17,) * 3, (20,) * 3, (21,) * 3, (23,) * 3, (24,) * 3, (26, 26), (30,) * 3]]
    # row-code MFMA (13^4: R = 1 and 42 k-steps)
    + [_c((7,) * 5, big=True, rot=True), _c((9,) * 4, rot=True), _c((11,) * 5, big=True, rot=True), _c((12,) * 4, rot=True),
       _c((15,) * 4), _c((12, 12, 10, 16)), _c((6, 6, 6, 12, 12), rot=True), _c((13,) * 4), _c((5,) * 5), _c((6,) * 5)]
    # wide codes
    + [_c((4,) * 6), _c((3,) * 10)]
    # grid (64^4: signature only)
    + [_c((n,) * 3) for n in (28, 32, 40, 48, 65)] + [_c((64,) * 4)]
    # k-fold and its neighbours
    + [_c(s) for s in [(9, 48, 30), (45, 20, 20), (30, 20, 20), (32, 16, 16), (64, 8, 8), (24, 20, 20), (22,) * 3, (2, 17, 17),
                       (25, 25, 40), (40, 12, 12), (26, 14, 14)]]
    # switch arms
    + [_c((13,) * 4, {"PCX_BARY_SEED": "0"}), _c((5,) * 5, {"PCX_BARY_SEED": "0"})]
    + [_c(s, {"PCX_BARY_GRID": v}) for s in [(30,) * 3, (7,) * 5] for v in ("0", "2")]
    + [_c((17,) * 3, {"PCX_BARY_SQ": "0"})]
    + [_c((11,) * 5, {"PCX_BARY_TAIL": v}, big=True) for v in ("0", "2")]
    + [_c((30,) * 3, {"PCX_BARY_GRID_PROD": "0"})]
    # ... 30^3 runs on the k-fold form: the grid switches on a shape the grid form takes as well
    + [_c((40,) * 3, {"PCX_BARY_GRID": v}) for v in ("0", "2")] + [_c((40,) * 3, {"PCX_BARY_GRID_PROD": "0"})]
)
PER_PROCESS = ("PCX_BARY_SQ",)          # read once per process: a child of their own


def case_id(case):
    name = "x".join(map(str, case["shape"]))
    return name + "".join(f"|{k}={v}" for k, v in sorted(case["env"].items()))


def group_of(case):
    """'default', 'perhandle' or the per-process switch setting the case needs."""
    for k in PER_PROCESS:
        if k in case["env"]:
            return f"{k}={case['env'][k]}"
    return "perhandle" if case["env"] else "default"


def grid_1d(n):
    """Chebyshev nodes of the first kind on [-1, 1] (ascending), their barycentric weights in closed form
    ((-1)^j sin((2j + 1) pi / 2n): no product that under- or overflows at n = 4096) and the differentiation matrix."""
    j = np.arange(n)
    theta = (2 * j + 1) * np.pi / (2 * n)
    x = -np.cos(theta)
    w = np.where(j % 2 == 0, 1.0, -1.0) * np.sin(theta)
    gap = x[:, None] - x[None, :]
    np.fill_diagonal(gap, 1.0)
    D = w[None, :] / (gap * w[:, None])
    np.fill_diagonal(D, 0.0)
    np.fill_diagonal(D, -D.sum(axis=1))
    return x, w, D


def model_arrays(shape):
    """nodes_cat, weights_cat, diffmat_cat and the seeded random tensor (flat, C order) of a shape."""
    grids = {n: grid_1d(n) for n in set(shape)}
    nodes = np.concatenate([grids[n][0] for n in shape])
    wts = np.concatenate([grids[n][1] for n in shape])
    diff = np.concatenate([grids[n][2].ravel() for n in shape])
    seed = int.from_bytes(hashlib.sha256(repr(tuple(shape)).encode()).digest()[:4], "little")
    tensor = np.random.default_rng(seed).standard_normal(int(np.prod(shape, dtype=np.int64)))
    return nodes, wts, diff, tensor


def _info(lib, L, h, name, count):
    buf = np.zeros(count, dtype=np.int32)
    L.check(getattr(lib, name)(h, L.p_i32(buf)), lib)
    return [int(v) for v in buf]


def _digest(lib, L, h, pts, specs):
    """SHA-256 of eval_multi_batch's output, evaluated twice: None when the two runs differ."""
    specs = L.i32(specs)
    seen = []
    for _ in range(2):
        out = np.full((pts.shape[0], specs.shape[0]), np.nan)
        L.check(lib.pcx_bary_eval_multi_batch(h, L.p_f64(pts), pts.shape[0], L.p_i32(specs), specs.shape[0], L.p_f64(out)), lib)
        seen.append(hashlib.sha256(out.tobytes()).hexdigest())
    return seen[0] if seen[0] == seen[1] else None


def _gemms(lib, L, h, specs, N):
    specs = L.i32(specs)
    cnt = np.zeros(1, dtype=np.int32)
    L.check(lib.pcx_bary_count_gemms(h, L.p_i32(specs), specs.shape[0], N, L.p_i32(cnt)), lib)
    return int(cnt[0])


def _unit(d, k, order=1):
    v = [0] * d
    v[k] = order
    return v


def measure(case, device=0):
    """The record of one case with the library as it is built now.  The case's per-handle switches are set in the
    environment around the create; per-process ones must be set already."""
    from pychebyshev_amd import _lib as L
    lib = L.load()
    shape, d = case["shape"], len(case["shape"])
    rec = {"id": case_id(case), "shape": shape, "env": case["env"]}
    nodes, wts, diff, tensor = model_arrays(shape)
    for k in PER_PROCESS:
        assert os.environ.get(k) == case["env"].get(k), f"{rec['id']}: {k} is read once per process"
    own = {k: v for k, v in case["env"].items() if k not in PER_PROCESS}
    os.environ.update(own)
    try:
        h = ctypes.c_void_p()
        rc = lib.pcx_bary_create(device, d, L.p_i32(L.i32(shape)), L.p_f64(nodes), L.p_f64(wts), L.p_f64(diff), L.p_f64(tensor),
                                 ctypes.byref(h))
    finally:
        for k in own:
            del os.environ[k]
    rec["rc"] = int(rc)
    if rc != 0:
        rec["error"] = L.last_error(lib)
        return rec
    try:
        rec["kernel_info"] = _info(lib, L, h, "pcx_bary_kernel_info", 6)
        rec["grid_info"] = _info(lib, L, h, "pcx_bary_grid_info", 4)
        rec["tail_info"] = _info(lib, L, h, "pcx_bary_tail_info", 6)[1:4]
        rec["set_kernel"] = [lib.pcx_bary_set_kernel(h, v) == 0 for v in (2, 3, 4, 5)]
        L.check(lib.pcx_bary_set_kernel(h, 0), lib)
        rng = np.random.default_rng(27)
        if tensor.size <= DIGEST_MAX_ELEMS:
            pts = rng.uniform(-1.0, 1.0, (N_SMALL, d))
            specs = [[0] * d, _unit(d, 0), _unit(d, d - 1)]
            rec["digest"] = _digest(lib, L, h, pts, specs)
            if rec["set_kernel"][0] and rec["kernel_info"][0] != 2:
                L.check(lib.pcx_bary_set_kernel(h, 2), lib)
                rec["digest_mfma"] = _digest(lib, L, h, pts, specs)
                L.check(lib.pcx_bary_set_kernel(h, 0), lib)
        if case.get("big"):
            pts = rng.uniform(-1.0, 1.0, (N_BIG, d))
            specs = [[0] * d, _unit(d, 0), _unit(d, 0, 2)]
            rec["gemms_big"] = _gemms(lib, L, h, specs, N_BIG)
            rec["digest_big"] = _digest(lib, L, h, pts, specs)
        if case.get("rot"):
            rec["gemms_rot"] = [_gemms(lib, L, h, [[0] * d, _unit(d, q)], N_BIG) for q in range(d)]
    finally:
        lib.pcx_bary_destroy(h)
    return rec


def measure_group(group):
    return [measure(c) for c in CASES if group_of(c) == group]


def measure_in_child(group, path):
    """Run this file as a fresh child that measures one group into `path` -> its records."""
    env = dict(os.environ)
    if "=" in group:
        k, v = group.split("=", 1)
        env[k] = v
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", group, "--json", path], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, f"group {group}: exit {res.returncode}\n{res.stdout[-4000:]}"
    with open(path) as fh:
        return json.load(fh)


def groups():
    seen = []
    for c in CASES:
        if group_of(c) not in seen:
            seen.append(group_of(c))
    return seen


def load(path=OUT):
    """id -> record of the committed fixture."""
    with np.load(path) as z:
        return {r["id"]: r for r in json.loads(str(z["records"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child")
    ap.add_argument("--json")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.child:
        with open(args.json, "w") as fh:
            json.dump(measure_group(args.child), fh)
        return
    import tempfile
    records, dropped = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for i, g in enumerate(groups()):
            for r in measure_in_child(g, os.path.join(tmp, f"g{i}.json")):
                unstable = [k for k in ("digest", "digest_mfma", "digest_big") if k in r and r[k] is None]
                (dropped if unstable else records).append(r)
                print(json.dumps(r), flush=True)
    if dropped:
        print("NOT WRITTEN (two runs of a digest differed):", [r["id"] for r in dropped])
    assert len(dropped) <= 2, "more than two cases have no stable digest: the digest approach does not hold"
    np.savez_compressed(args.out, records=np.array(json.dumps(records)))
    print(f"wrote {len(records)} records to {args.out}")


if __name__ == "__main__":
    main()
