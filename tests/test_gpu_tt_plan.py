"""Every evaluation form and rank class of the tensor-train handle against records taken before the planner was split
from pcx_tt_create.

tests/golden/g36_tt_plans.npz (tests/golden/generate_golden_tt_plans.py wrote it on an MI355X) holds, per case, the
return code and error text of create, which of set_kernel(1..4) are accepted, and SHA-256 digests of eval_batch (auto and
every accepted variant) and of eval_multi_batch (value, one first-order and one second-order spec).  Each case is measured
again with the library under test, by the generator's own code, and compared exactly: the same acceptances, the same
bytes.  Where two forms' recorded digests coincide the case does not pin auto's choice; tests/test_tt_plan_host.py does."""
import pytest

import generate_golden_tt_plans as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return G.load()


def test_every_case_of_the_generator_is_in_the_fixture(recorded):
    assert sorted(recorded) == sorted(c["id"] for c in G.CASES)


@pytest.mark.parametrize("case", G.CASES, ids=[c["id"] for c in G.CASES])
def test_case_matches_the_record(recorded, case):
    got = G.measure(case)
    assert not G.unstable(got), "two runs of one digest differ"
    assert got == recorded[case["id"]]


def test_the_record_covers_every_form_and_class(recorded):
    """auto's digest equals the digest of the form the case is named for, and of no other form where they differ"""
    def auto_is(cid, variant):
        dg = recorded[cid]["digest"]
        return dg["0"] == dg[str(variant)] and all(dg[v] != dg["0"] for v in dg if v not in ("0", str(variant)))

    assert auto_is("r4_n8", 4) and auto_is("r12_n12", 4) and auto_is("r13_n9", 4) and auto_is("mixed_order", 4)
    assert auto_is("r16_n10", 1) and auto_is("r5_n17", 2) and auto_is("r12_n32_d3", 2)
    for cid in ("r5_n33", "r12_n32_d5", "r17_n6", "r32_n5", "r33_n5", "r64_n4", "mixed_r20"):
        assert recorded[cid]["set_kernel"] == [True, False, False, False], cid
    assert recorded["r65_n4"]["set_kernel"] == [False] * 4 and list(recorded["r65_n4"]["digest"]) == ["0"]
    assert [recorded[cid]["rc"] for cid in ("r4097", "lds_over", "bad_boundary", "bad_domain", "bad_order")] == [-4, -4, -1, -1, -1]
