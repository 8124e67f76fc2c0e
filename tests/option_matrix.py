"""One row per execution option (lumo_amd._ffi.OPTIONS, include/lumo_amd.h LUMO_OPT_*): its range as
the header documents it and where the suite renders with it away from its default.

tests/test_option_coverage.py (no GPU) holds the table to _ffi.OPTIONS, to the option table of
ctx.hip (kOpts) and to the test functions it names; tests/test_gpu_options.py walks the ranges on a
device.  A new option needs a row, and a row needs a parity test that renders with the option set.

Row: name -> Row(lo, hi, values, default, covered, exempt)
  lo, hi    lowest and highest accepted value (hi None: it comes from the device, top_kb)
  values    the accepted values where they are not the whole range, else None
  default   the default of a fresh context (None: set from the device at creation)
  covered   [(non-default value, "tests/file.py::test_function")]: a GPU test that renders with that
            value and compares with the oracle; the function's source names the option
  exempt    why no parity test sets it (then covered may be empty)
"""
from collections import namedtuple

Row = namedtuple("Row", "lo hi values default covered exempt")

BIG = 1 << 31       # tail_below, bdpt_tail: path counts
GRID_MAX = 1 << 20  # lds_grid, top_grid
STACK_CLASSES = (4, 8, 16, 24, 32, 48, 64)  # launch.h STACK_CLASSES

_P, _S, _B, _O = ("tests/test_gpu_parity.py::", "tests/test_gpu_scale.py::", "tests/test_gpu_bdpt.py::",
                  "tests/test_gpu_options.py::")

OPTION_MATRIX = {
    "timing": Row(0, 1, None, 0, [], "timing: records HIP events around launches; no kernel or schedule differs"),
    "lds_staging": Row(0, 1, None, 1, [(0, _S + "test_kernel_variants")], None),
    "top_staging": Row(0, 1, None, 1, [(0, _S + "test_top_staging_budgets")], None),
    "fused": Row(-1, 1, None, -1, [(0, _P + "test_bounce_modes_match_oracle"),
                                   (1, _P + "test_bounce_modes_match_oracle")], None),
    "tail_below": Row(0, BIG, None, 1 << 16, [(0, _P + "test_bounce_modes_match_oracle"),
                                              (300, _P + "test_bounce_modes_match_oracle")], None),
    "pipeline": Row(0, 3, None, 3, [(0, _P + "test_bounce_modes_match_oracle"),
                                    (1, _P + "test_bounce_modes_match_oracle"),
                                    (2, _P + "test_bounce_modes_match_oracle")], None),
    "heads": Row(0, 64, None, 0, [(4, _P + "test_head_bounce_counts_match_oracle"),
                                  (8, _P + "test_head_bounce_counts_match_oracle")], None),
    "merge_passes": Row(0, 8, None, 0, [(3, _P + "test_merged_passes_match_oracle"),
                                        (3, _O + "test_tail_bounces")], None),
    "dyn_fetch": Row(0, 1, None, 0, [(1, _P + "test_fused_fetch_modes_match_oracle")], None),
    "bounce_threads": Row(64, 256, (64, 128, 256), 256, [(64, _O + "test_fused_bounce_threads"),
                                                        (128, _O + "test_fused_bounce_threads"),
                                                        (64, _O + "test_bounce_threads_with_tail_mid_pass"),
                                                        (128, _O + "test_bounce_threads_with_tail_mid_pass"),
                                                        (64, _O + "test_bounce_threads_decide_the_schedule")], None),
    "split_pipe": Row(1, 4, None, 4, [(2, _S + "test_split_pipeline_passes_in_flight")], None),
    "split_groups": Row(1, 4, None, 2, [(4, _S + "test_split_pipeline_passes_in_flight")], None),
    "bdpt_tail": Row(0, BIG, None, 1 << 16, [(0, _B + "test_bdpt_tiles_and_splats"),
                                             (300, _B + "test_bdpt_tiles_and_splats")], None),
    "bounce_ahead": Row(1, 15, None, 3, [(1, _O + "test_bounce_ahead"), (15, _O + "test_bounce_ahead"),
                                         (15, _O + "test_bounce_ahead_many_passes")], None),
    "lds_grid": Row(1, GRID_MAX, None, None, [(7, _P + "test_fused_fetch_modes_match_oracle")], None),
    "top_grid": Row(1, GRID_MAX, None, None, [(1, _O + "test_top_grid_trace"), (3, _O + "test_top_grid_trace"),
                                              (1, _O + "test_top_grid_render"), (3, _O + "test_top_grid_render"),
                                              (1, _O + "test_top_grid_bdpt"), (3, _O + "test_top_grid_bdpt")], None),
    "top_kb": Row(0, None, None, None, [(8, _S + "test_top_staging_budgets"), (24, _S + "test_top_budget_caps_lds")],
                  None),
    "kd_lds": Row(0, 64, None, 8, [(4, _S + "test_kd_treelets_in_lds"), (0, _S + "test_kd_treelets_in_lds")], None),
    "stack_class": Row(0, 64, (0,) + STACK_CLASSES, 0, [(64, _S + "test_kernel_variants")], None),
    "full_kernels": Row(0, 1, None, 0, [(1, _S + "test_kernel_variants")], None),
    "poison": Row(0, 1, None, 0, [], "poison: the whole test session runs with it on (conftest, LUMO_POISON)"),
    "tail_priority": Row(0, 1, None, 0, [(1, _O + "test_tail_priority")], None),
    "top_kd": Row(0, 1, None, 1, [(0, _S + "test_kd_treelets_in_lds")], None),
    "tail_bounces": Row(-1, 16, None, -1, [(0, _O + "test_tail_bounces"), (1, _O + "test_tail_bounces"),
                                           (3, _O + "test_tail_bounces"), (16, _O + "test_tail_bounces")], None),
    "film_first": Row(0, 1, None, 0, [(1, _O + "test_film_first")], None),
    "bdpt_top": Row(0, 1, None, 1, [(0, _B + "test_bdpt_top_visibility_matches_oracle")], None),
    "bdpt_groups": Row(1, 4, None, 2, [(1, _B + "test_bdpt_task_groups"), (4, _B + "test_bdpt_task_groups")], None),
    "ray_sort": Row(-1, 2, None, -1, [(1, _S + "test_ray_sort_matches_oracle"), (2, _B + "test_bdpt_walk_ray_sort")],
                    None),
    "accel": Row(0, 1, None, 0, [(1, "tests/test_gpu_wide.py::test_wide_cornell_fused_tiles")] +
                 [(1, "tests/test_gpu_wide_forms.py::" + t) for t in (
                     "test_wide_kernel_variants", "test_wide_split_kernels_staged", "test_wide_bounce_modes_small_dragon",
                     "test_wide_fused_pipeline_staged", "test_wide_top_prefix_edges", "test_wide_whole_tree_in_top",
                     "test_wide_top_cut_in_blas", "test_wide_split_pipeline", "test_wide_bdpt_walk_forms",
                     "test_wide_bdpt_top_visibility", "test_wide_bdpt_task_groups",
                     "test_wide_bdpt_long_subpaths_are_rerun", "test_wide_bdpt_walk_ray_sort",
                     "test_wide_refusal_and_boundary")], None),
}
