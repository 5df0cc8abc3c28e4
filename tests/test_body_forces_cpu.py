"""CPU: external forces on the rigid bodies (bez_sim_apply_body_forces) -- the C ABI entry and its constants, the additive-only ABI,
the per-body centre-of-mass table, the Python argument checks, and the step kernels: every instantiation builds for gfx950 and the
instantiations that existed before keep their register / spill / scratch / LDS figures exactly (tests/golden/step_kernel_resources.txt,
recorded from the build before the force-carrying instantiations were added)."""
import ctypes as C
import concurrent.futures as cf
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

from bez_isaacgym_amd import abi
from tests.kernel_resources import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "bez_sim.h")).read()
GEN = open(os.path.join(ROOT, "bez_isaacgym_amd", "csrc", "bez_model_gen.h")).read()
CSRC = os.path.join(ROOT, "bez_isaacgym_amd", "csrc")
TUS = ("bez_step_ws8", "bez_step_ws8q", "bez_step_lane")
RESOURCES = os.path.join(ROOT, "tests", "golden", "step_kernel_resources.txt")


def test_header_declares_the_entry_and_the_binding_lists_it():
    assert re.search(r"int bez_sim_apply_body_forces\(BezSim\* sim, const float\* forces_dev, const float\* torques_dev, "
                     r"const float\* positions_dev, int32_t space,\s+void\* stream\);", HDR)
    from bez_isaacgym_amd.sim import EXPORTS
    assert "bez_sim_apply_body_forces" in EXPORTS


def test_space_constants_match():
    assert int(re.search(r"#define BEZ_SPACE_ENV (\d+)", HDR).group(1)) == abi.SPACE_ENV == 0
    assert int(re.search(r"#define BEZ_SPACE_LOCAL (\d+)", HDR).group(1)) == abi.SPACE_LOCAL == 1
    for v, want in (("env", 0), ("ENV", 0), ("local", 1), ("Local", 1), (0, 0), (1, 1)):
        assert abi.body_force_space(v) == want
    for bad in ("world", "", 2, -1, 1.0, None, True):
        with pytest.raises(ValueError):
            abi.body_force_space(bad)


def test_abi_is_unchanged():
    """additive only: ABI version 5, 17 tensors, the BezSimConfig layout and bez_sim_default_config's bytes as before"""
    assert int(re.search(r"#define BEZ_SIM_ABI_VERSION (\d+)", HDR).group(1)) == abi.ABI_VERSION == 5
    assert re.findall(r"BEZ_TENSOR_COUNT = (\d+)", HDR) == ["17"] and abi.TENSOR_COUNT == 17
    assert C.sizeof(abi.BezSimConfig) == 304
    from bez_isaacgym_amd.build import build
    from bez_isaacgym_amd.sim import load_library
    build()
    lib = load_library()
    cfg = abi.BezSimConfig()
    assert lib.bez_sim_default_config(C.byref(cfg), 4096) == 0
    digest = hashlib.sha256(bytes(cfg)).hexdigest()
    assert digest == _DEFAULT_CONFIG_SHA256, digest
    assert cfg.flags == abi.FLAG_IMU_PREV_ALIAS | abi.FLAG_NONFINITE_GUARD   # no new default flag bit


# sha256 of the 304 bytes bez_sim_default_config(4096) wrote before this feature (recorded from that build)
_DEFAULT_CONFIG_SHA256 = "ec6306b2486db996b7db67fd440a39f6ec77a2239e0a0adf4d11cc830c7fff0a"


def _table(name, text=GEN):
    m = re.search(r"%s\[[^\]]*\]\[3\] = \{(.*?)\};" % re.escape(name), text, re.S)
    return np.array([float(x) for x in re.findall(r"[-+0-9.eE]+", m.group(1))]).reshape(-1, 3)


def test_body_com_table_matches_the_urdf_fixture():
    """BEZ_BODY_COM (and the model JSON's body_com) = the inertial origin of every rigid body of tests/golden/urdf_bodies.json"""
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "urdf_bodies.json")))["bodies"]
    m = json.load(open(os.path.join(ROOT, "bez_isaacgym_amd", "model", "bez_model.json")))
    by_name = {b["name"]: b["com"] for b in fx}
    com = _table("BEZ_BODY_COM")
    assert com.shape == (len(m["body_names"]), 3) == (21, 3)
    assert len(by_name) == 21
    for i, name in enumerate(m["body_names"]):
        np.testing.assert_allclose(com[i], by_name[name], rtol=0, atol=1e-12, err_msg=name)
        np.testing.assert_allclose(m["body_com"][i], by_name[name], rtol=0, atol=1e-12, err_msg=name)
    # cleats asset: the same bodies keep their centres, the eight cleats are their own bodies
    com_cl = _table("BEZ_BODY_COM_CL")
    assert com_cl.shape == (29, 3)
    for i, name in enumerate(m["cleats"]["body_names"]):
        if name in by_name:
            np.testing.assert_allclose(com_cl[i], by_name[name], rtol=0, atol=1e-12, err_msg=name)
    np.testing.assert_allclose(com_cl, np.asarray(m["cleats"]["body_com"]), rtol=0, atol=1e-12)


class _FakeLib:
    def __init__(self):
        self.calls = []

    def bez_sim_apply_body_forces(self, h, f, t, x, space, stream):
        self.calls.append((f, t, x, space))
        return 0


def _bare_sim(n=4, nb=22):
    """a BezSim without a device: the argument checks run before anything reaches the library"""
    from bez_isaacgym_amd.sim import BezSim
    s = BezSim.__new__(BezSim)
    s.lib, s.h, s.num_envs, s.num_bodies, s.device = _FakeLib(), None, n, nb, torch.device("cpu")
    s._stream = lambda: None
    return s


def test_python_argument_checks():
    from bez_isaacgym_amd.sim import BezSimError
    s = _bare_sim()
    good = torch.zeros((4, 22, 3))
    s.apply_body_forces(forces=good, space="local")
    s.apply_body_forces(forces=good.reshape(88, 3), torques=good, positions=None, space=abi.SPACE_ENV)
    assert [c[3] for c in s.lib.calls] == [1, 0]
    assert s.lib.calls[1][2] is None and s.lib.calls[1][0] is not None
    bad = [dict(forces=torch.zeros((4, 21, 3))), dict(forces=torch.zeros((88, 4))), dict(forces=torch.zeros(264)),
           dict(forces=torch.zeros((4, 22, 3), dtype=torch.float64)), dict(torques=torch.zeros((4, 22, 3), dtype=torch.float16)),
           dict(forces=good, positions=torch.zeros((3, 22, 3))), dict(forces=torch.zeros((4, 3, 22)).transpose(1, 2)),
           dict(forces=np.zeros((4, 22, 3), np.float32))]
    for kw in bad:
        with pytest.raises(BezSimError):
            s.apply_body_forces(**kw)
    for space in ("world", 3, -1):
        with pytest.raises(ValueError):
            s.apply_body_forces(forces=good, space=space)
    assert len(s.lib.calls) == 2   # nothing that failed a check reached the library
    # bez_walk / bez_orient: 21 bodies
    w = _bare_sim(nb=21)
    w.apply_body_forces(forces=torch.zeros((4, 21, 3)))
    with pytest.raises(BezSimError):
        w.apply_body_forces(forces=good)


def test_vec_task_entry_points_forward():
    from bez_isaacgym_amd.tasks.base.vec_task import VecTask
    calls = []

    class _S:
        def apply_body_forces(self, **kw):
            calls.append(kw)
    class _T(VecTask):
        def pre_physics_step(self, actions): pass
        def post_physics_step(self): pass
    t = _T.__new__(_T)
    t.sim = _S()
    f, x, tq = object(), object(), object()
    assert t.apply_rigid_body_force_tensors(f, tq, "local") is True
    assert t.apply_rigid_body_force_at_pos_tensors(f, x) is True
    assert calls == [dict(forces=f, torques=tq, positions=None, space="local"), dict(forces=f, torques=None, positions=x, space="env")]


# ---- the kernels


def _is_ext(name):
    return name.endswith("Lb1EEEvNS_6ParamsE") and "step_kernel" in name and _nargs(name) in (5, 6)


def _nargs(name):
    m = re.search(r"step_kernel(?:_ws8)?I((?:Lb[01]E)+)EEv", name)
    return len(m.group(1)) // 4 if m else 0


def _as_before(name):
    """the symbol the same instantiation had before the EXT parameter was appended (EXT = false)"""
    return name.replace("Lb0EEEvNS_6ParamsE", "EEvNS_6ParamsE")


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    d = tmp_path_factory.mktemp("kres")
    with cf.ThreadPoolExecutor(len(TUS)) as ex:
        res = list(ex.map(lambda tu: kernel_resources(os.path.join(CSRC, tu + ".hip"), str(d)), TUS))
    return dict(zip(TUS, res))


def test_every_instantiation_builds_for_gfx950(resources):
    ws8, ws8q, lane = (resources[t] for t in TUS)
    for tab, want in ((ws8, 6 + 4), (ws8q, 6 + 4), (lane, 12 + 4)):
        assert len(tab) == want, sorted(tab)
    for tab in (ws8, ws8q, lane):
        ext = [k for k in tab if _is_ext(k)]
        assert len(ext) == 4, ext   # (full step, physics only) x (default asset, cleats), built with the per-env parameter loads


def test_existing_instantiations_keep_their_resources(resources):
    want = {}
    for line in open(RESOURCES):
        if line.strip() and not line.startswith("#"):
            tu, name, *vals = line.split()
            want[(tu, name)] = tuple(int(v) for v in vals)
    got = {(tu, _as_before(k)): v for tu in TUS for k, v in resources[tu].items() if not _is_ext(k)}
    assert set(got) == set(want), set(got) ^ set(want)
    for key in want:
        assert got[key] == want[key], (key, got[key], want[key])
