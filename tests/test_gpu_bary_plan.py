"""Every decision branch of handle creation against records taken before the planner was split from pcx_bary_create.

tests/golden/g27_bary_plans.npz (tests/golden/generate_golden_bary_plans.py wrote it on an MI355X) holds, per case, the
plan signature (kernel_info, grid_info, tail_info[1..3], the set_kernel acceptances), count_gemms of the large spec
sets and SHA-256 digests of eval_multi_batch's outputs.  Each case is measured again with the library under test, by
the generator's own code, and compared exactly: the same plan, the same bytes.  The default cases run in this process;
switches the library reads once per process, and the per-handle ones, run in two children (as in the generator)."""
import numpy as np
import pytest

import generate_golden_bary_plans as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return G.load()


@pytest.fixture(scope="module")
def measured(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bary_plans")
    recs = []
    for i, group in enumerate(G.groups()):
        recs += G.measure_group(group) if group == "default" else G.measure_in_child(group, str(tmp / f"g{i}.json"))
    return {r["id"]: r for r in recs}


@pytest.mark.parametrize("cid", [G.case_id(c) for c in G.CASES])
def test_case_matches_the_record(recorded, measured, cid):
    want, got = recorded[cid], measured[cid]
    if "digest" not in want and want["rc"] == 0:
        assert int(np.prod(want["shape"], dtype=np.int64)) > G.DIGEST_MAX_ELEMS       # 64^4: the signature only
    assert got == want


def test_rotated_models_exist_where_they_did(recorded, measured):
    """bary_rot asks the planner before it builds anything: 11^5 still shares a GEMM between price and delta along every
    dimension (q > 0: on the rotated sub-model), and the shapes whose rotation has no slab plan still share none."""
    with_rot = recorded["11x11x11x11x11"]["gemms_rot"]
    assert with_rot == [1] * 5, "the record no longer shows a rotated model per dimension"
    assert measured["11x11x11x11x11"]["gemms_rot"] == with_rot
    without = [cid for cid, r in recorded.items() if r.get("gemms_rot") and all(g == 2 for g in r["gemms_rot"][1:])]
    assert "7x7x7x7x7" in without
    for cid in without:
        assert measured[cid]["gemms_rot"] == recorded[cid]["gemms_rot"], cid
