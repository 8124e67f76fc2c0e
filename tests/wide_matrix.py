"""One row per traversal launcher of lumo_amd/csrc/device/launch.h: the staging forms the launcher has
and the GPU parity test that runs each form in the wide accel mode (LUMO_OPT_ACCEL 1, stack class 0,
the eighth instantiation of every launcher).

Forms (launch.h TravLaunch, kernels.hip launch_trav):
  lds    the whole packed scene staged in LDS (TravLaunch::lds; scenes up to 48 KiB)
  top    the TOP set in LDS: the object records and a breadth-first prefix of the wide nodes
         (TravLaunch::top; only the launchers kernels.hip calls with allow_top, and lumo_trace)
  plain  every node read from HBM

tests/test_wide_coverage.py (no GPU) holds the table to the launchers declared in launch.h, to the
forms their definitions (inst_pt.hip, inst_bd.hip) branch on, and to the test functions it names; each
named test's source names `accel`.  A new launcher needs a row, and a row needs a wide-mode test per form.
"""
_F = "tests/test_gpu_wide_forms.py::"

WIDE_MATRIX = {
    # BDPT walk bounces ahead of k_bdpt_step (bdpt_tail 0 / 300)
    "launch_closest": {"lds": _F + "test_wide_bdpt_walk_forms", "plain": _F + "test_wide_bdpt_top_visibility"},
    # split bounces: Cornell staged with fused 0; Cornell with staging off has no TOP set either (plain)
    "launch_closest_q": {"lds": _F + "test_wide_split_kernels_staged", "top": _F + "test_wide_top_prefix_edges",
                         "plain": _F + "test_wide_kernel_variants"},
    "launch_shadow_q": {"lds": _F + "test_wide_split_kernels_staged", "top": _F + "test_wide_top_prefix_edges",
                        "plain": _F + "test_wide_kernel_variants"},
    "launch_bounce_q": {"lds": _F + "test_wide_fused_pipeline_staged",
                        "plain": _F + "test_wide_bounce_modes_small_dragon"},
    "launch_trace": {"top": _F + "test_wide_top_prefix_edges", "plain": _F + "test_wide_top_prefix_edges"},
    "launch_bdpt_step": {"plain": _F + "test_wide_bdpt_walk_forms"},
    "launch_bdpt_tail": {"lds": _F + "test_wide_bdpt_walk_forms", "plain": _F + "test_wide_bdpt_top_visibility"},
    "launch_bdpt_redo": {"lds": _F + "test_wide_bdpt_long_subpaths_are_rerun",
                         "plain": _F + "test_wide_bdpt_top_visibility"},
    "launch_bdpt_trace_a": {"lds": _F + "test_wide_bdpt_walk_forms", "plain": _F + "test_wide_bdpt_top_visibility"},
    "launch_bdpt_vis": {"lds": _F + "test_wide_bdpt_walk_forms", "top": _F + "test_wide_bdpt_top_visibility",
                        "plain": _F + "test_wide_bdpt_top_visibility"},
}
