"""CPU: the Python binding's argument handling (BezSim's query calls and apply_body_forces, the parsers and parameter builders of abi.py)
against tests/golden/binding_calls.json, the record tests/binding_record.py produced on the commit before the binding was folded
into shared resolvers.  One line of that file was then edited by hand: limb_ik(offsets=3), which used to leak a bare TypeError and
is now refused like operational_space(offsets=3)."""
import json
import os

import pytest

from tests import binding_record

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_calls.json")


@pytest.fixture(scope="module")
def rec():
    return binding_record.record()


def test_record_equals_the_golden_record(rec):
    from bez_isaacgym_amd import sim
    want = json.load(open(GOLDEN))
    assert sorted(rec) == sorted(want)
    assert sim.EXPORTS == [s.split(":")[0] for s in want["signatures"]]
    for key in want:
        for k, (e, w) in enumerate(zip(rec[key], want[key])):
            assert binding_record.line(e) == w, "%s[%d] differs" % (key, k)
        assert len(rec[key]) == len(want[key]), key


# one fragment per `raise` the table reaches: sim.py's own, and those of the abi parsers and parameter builders behind them
RAISES = ("expected a contiguous torch.float32 tensor on cpu, got torch.float64 on cpu", "got torch.float32 on meta", "got torch.float32 on cpu",
          "expected a torch tensor, got ndarray", "udot: expected shape (3, 24), got", "targets: expected shape (3, 5, 7) or (15, 7), got",
          "forward_dynamics: bias must be a subset", "forward_dynamics: bias is 0 and force is None",
          "operational_space: want holds", "operational_space: nothing is wanted", "operational_space: 'lambda' with fixed_base",
          "operational_space: offsets must be (5, 3) or None", "operational_space: offsets[4][1] must be finite", "operational_space: fixed_base must be",
          "generalized_forces: forces and torques are both None", "generalized_forces: at='origin' is the point of application",
          "at must be 'com' or 'origin'", "space must be 'env' or 'local'", "space must be SPACE_ENV (0) or SPACE_LOCAL (1)",
          "limb_ik: weights must be (5, 2)", "limb_ik: weights[2][1] must be finite and >= 0", "limb_ik: offsets must be (5, 3) or None",
          "limb_ik: offsets[2][0] must be finite", "limb_ik: damping must be", "limb_ik: max_step is NaN", "limb_ik: iters must be an integer",
          "limb_ik: space must be 'env' or 'root'", "limb_ik: space must be IK_SPACE_ENV (0) or IK_SPACE_ROOT (1)",
          "proximity: want holds", "proximity: nothing is wanted", "libbez_sim call failed (-3)")


def test_the_table_reaches_every_refusal(rec):
    refused = [e for e in rec["calls"] if "refused" in e]
    assert [e["sim"] for e in refused if "library_calls" in e] == ["the library fails"] * 3   # every other refusal left the library untouched
    assert binding_record.refusals({"calls": [e for e in refused if "library_calls" not in e]}) == {
        "inverse_dynamics": 14, "forward_dynamics": 25, "operational_space": 50, "centroidal": 13, "body_accelerations": 22,
        "generalized_forces": 55, "limb_ik": 54, "proximity": 26, "apply_body_forces": 34}
    assert {e["refused"][0] for e in refused} == {"BezSimError", "ValueError"}
    messages = [e["refused"][1] for e in refused]
    for fragment in RAISES:
        assert any(fragment in m for m in messages), fragment
    # every accepted call is one library call, and a buffer the sim allocated once stays where it is
    done = [e for e in rec["calls"] if "refused" not in e]
    assert all(len(e["library"]) == 1 and "moved" not in e for e in done)
    plain = {m: m + "()" for m in binding_record.QUERIES}
    plain.update(limb_ik="limb_ik(targets=float32(3, 5, 7), weights=W_ALL)", generalized_forces="generalized_forces(forces=float32(3, 22, 3))")
    for method, call in plain.items():   # the second and every later call: the first call's scratch buffers at the same addresses, nothing new
        first, *later = [e for e in done if e["call"] == call and e["sim"] == "22 bodies"]
        assert later and all("allocated" not in e and e["library"] == first["library"] for e in later), method
        assert any(a.startswith("scratch:" + method) for a in first["library"][0][1] if isinstance(a, str)), method
