"""Shared test helpers live in support modules (tests/sim_cfg.py, state_sets.py, gpu_util.py, the *_numpy.py / *_ref.py references, ...):
no file under tests/ or tools/, nor bench.py, imports a module named tests.test_*.

LEGACY lists the imports that stand inside the bodies of test functions and fixtures written before this rule.  Each still resolves,
mostly to a name its module now imports from a support module.  The list may only shrink: an entry goes when its test is next edited,
and an entry that no longer matches an import fails the test as well."""
import ast
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_AGENT = ("tests.test_gpu_round2",)
_CFG = ("tests.test_tasks",)
_RES = ("tests.test_body_forces_cpu",)
_PRESSED = ("tests.test_oracle_round6",)
# {file under tests/: {test function or fixture: the test modules its body imports}}
LEGACY = {
    "test_body_accelerations_cpu.py": {"test_the_kernel_of_both_assets_has_no_spills_and_no_scratch": _RES},
    "test_dof_force_cpu.py": {"resources": _RES, "test_restated_net_joint_force_is_the_inverse_dynamics_torque": _PRESSED},
    "test_dynamics_cpu.py": {"test_J_ref_routes_agree_and_have_the_documented_structure": ("tests.test_state_tensors_cpu",)},
    "test_generalized_forces_cpu.py": {"test_duality_with_the_finite_difference_jacobian": ("tests.test_state_tensors_cpu",),
                                       "test_the_kernel_of_both_assets_has_no_spills_and_no_scratch": _RES},
    "test_gpu_episode_stats.py": {"test_reward_terms_twin": ("tests.test_gpu_nonfinite_guard",)},
    "test_gpu_generalized_forces.py": {"test_closure_on_the_step": _PRESSED,
                                       "test_duality_with_the_jacobian_tensor_and_power": ("tests.test_gpu_dynamics",)},
    "test_gpu_inverse_dynamics.py": {"test_equation_of_motion_closes_on_the_step": _PRESSED},
    "test_gpu_limb_ik.py": {"test_duality_with_the_jacobian_tensor": ("tests.test_gpu_dynamics",)},
    "test_gpu_ppo_fused.py": {"test_fused_and_plain_optimiser_step_agree": _AGENT,
                              "test_segmented_graphs_equal_the_monolithic_update": _AGENT,
                              "test_train_forward_kernel_and_manual_backward_match_autograd_path": _AGENT,
                              "test_training_is_bit_reproducible": _AGENT},
    "test_gpu_round2.py": {"test_fused_step_kernels_agree": _CFG, "test_ws_kernel_post_physics_pinned_against_lane_kernel": _CFG},
    "test_gpu_round3.py": {"test_walk_goal_draw_advances_under_graph_replay": _CFG},
    "test_gpu_round4.py": {"test_dataset_prep_in_four_launches_equals_the_separate_launches": _AGENT,
                           "test_eager_work_and_checkpoint_saves_between_graph_replays_change_nothing": _AGENT,
                           "test_loss_in_front_of_the_backward_chain_changes_nothing": _AGENT,
                           "test_rollout_bookkeeping_inside_the_policy_launch_changes_nothing": _AGENT},
    "test_gpu_round5.py": {"test_dof_sweep_hip": ("tests.test_scenarios",),
                           "test_dr_hand_out_can_be_taken_back": ("tests.test_gpu_round3",),
                           "test_external_weight_writes_reach_the_mfma_kernels": _AGENT,
                           "test_fixed_base_hip_equals_oracle_and_the_torso_does_not_move": ("tests.test_scenarios",),
                           "test_pipelined_epochs_train_to_the_same_bits_and_report_the_same_numbers": _AGENT},
    "test_gpu_round6.py": {"test_lane_group_kernel_at_other_substep_counts": _CFG},
    "test_limb_ik_cpu.py": {"test_the_kernel_of_both_assets_has_no_spills_and_no_scratch": _RES},
    "test_nonfinite_guard_cpu.py": {"test_epoch_row_carries_nonfinite_resets": ("tests.test_ppo_cpu",),
                                    "test_epoch_row_without_counters_reports_zero": ("tests.test_ppo_cpu",)},
    "test_ppo_cpu.py": {"test_epoch_report_layout_is_pinned_and_grows_with_mini_epochs":
                        ("tests.test_dof_force_cpu", "tests.test_episode_stats_cpu", "tests.test_nonfinite_guard_cpu")},
}


def _test_modules(node):
    """the tests.test_* modules a node imports: import / from-import statements, __import__ and import_module calls with a literal"""
    if isinstance(node, ast.ImportFrom) and node.level == 0:
        names = [node.module or ""] + ["%s.%s" % (node.module, a.name) for a in node.names]
    elif isinstance(node, ast.Import):
        names = [a.name for a in node.names]
    elif (isinstance(node, ast.Call) and getattr(node.func, "id", getattr(node.func, "attr", None)) in ("__import__", "import_module")
          and node.args and isinstance(node.args[0], ast.Constant) and isinstance(node.args[0].value, str)):
        names = [node.args[0].value]   # ("tests.conftest" is no test module: the three free_port look-ups pass)
    else:
        return []
    return sorted({".".join(n.split(".")[:2]) for n in names if n.startswith("tests.test_")})


def _edges(path):
    """[(enclosing test function or fixture of a test file, or None; imported test module; line)]"""
    guarded = os.path.basename(path).startswith("test_") and os.path.basename(os.path.dirname(path)) == "tests"
    out = []

    def walk(node, owner):
        for ch in ast.iter_child_nodes(node):
            inner = owner
            if guarded and owner is None and isinstance(ch, (ast.FunctionDef, ast.AsyncFunctionDef)) and (
                    ch.name.startswith("test_") or any("fixture" in ast.dump(d) for d in ch.decorator_list)):
                inner = ch.name
            out.extend((owner, m, ch.lineno) for m in _test_modules(ch))
            walk(ch, inner)

    walk(ast.parse(open(path).read()), None)
    return out


def test_no_file_imports_a_test_module():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py"))) + [os.path.join(ROOT, "bench.py")]
    assert len(files) > 100
    bad, seen = [], set()
    for path in files:
        legacy = LEGACY.get(os.path.basename(path), {}) if os.path.dirname(path).endswith("tests") else {}
        for owner, module, line in _edges(path):
            if module in legacy.get(owner, ()):
                seen.add((os.path.basename(path), owner, module))
            else:
                bad.append("%s:%d imports %s" % (os.path.relpath(path, ROOT), line, module))
    assert not bad, bad
    stale = sorted({(f, fn, m) for f, fns in LEGACY.items() for fn, ms in fns.items() for m in ms} - seen)
    assert not stale, stale
