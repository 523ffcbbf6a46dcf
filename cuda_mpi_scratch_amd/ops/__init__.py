"""Device ops: thin wrappers over the gfx950 HIP kernels (csrc/kernels), with
exact CPU reference implementations for CPU tensors."""
from .cg import (CgWorkspace, cg_apply, cg_apply_reference, cg_check_operator, cg_check_sides,  # noqa: F401
                 cg_reference, cg_start, cg_start_reference, cg_update, cg_update_reference, ghosted, neumann_sides,
                 side_codes)
from .dot import DotWorkspace, dot  # noqa: F401
from .exact import (box_exact_reference, jacobi_sum_block_reference, stencil5_exact_block_reference,  # noqa: F401
                    stencil5_exact_periodic_reference, stencil5_exact_reference)
from .fill import fill, fill_random, fill_region, random_values  # noqa: F401
from .heat import (cg_heat_start, heat_coefficients, heat_rhs_reference, heat_start_reference,  # noqa: F401
                   heat_step_reference, pcg_heat_start)
from .multigrid import (mg_coarse_plan, mg_coarse_solve, mg_coarse_solve_reference, mg_plan_levels,  # noqa: F401
                        mg_prolong_add, mg_prolong_add_reference, mg_prolong_reference, mg_residual_reference,
                        mg_residual_restrict, mg_residual_restrict_reference, mg_restrict_reference, mg_smooth,
                        mg_smooth_reference, mg_smoother_table, multigrid_vcycle_reference)
from .pcg import (PcgPlan, PcgWorkspace, chebyshev_cycle_interval, level_sides, mgp_coarse_solve,  # noqa: F401
                  mgp_coarse_solve_reference, mgp_prolong_add, mgp_prolong_add_reference, mgp_residual_restrict,
                  mgp_residual_restrict_reference, mgp_smooth, mgp_smooth_reference, pcg_apply, pcg_coarse_interval,
                  pcg_coarse_plan, pcg_plan_levels, pcg_plan_levels_twin, pcg_precondition_reference, pcg_reference,
                  pcg_start, pcg_update)
from .relaxation import (chebyshev_cycle, fma, jacobi_held_levels_reference, relaxation_spectrum,  # noqa: F401
                         stencil5_tb_held_levels, stencil5_tb_levels)
from .source import jacobi_source_per_step_reference, source_correction_reference  # noqa: F401
from .stencil import (HOLD_BOTTOM, HOLD_LEFT, HOLD_RIGHT, HOLD_TOP, box_reference,  # noqa: F401
                      jacobi_held_reference, jacobi_reference_global, jacobi_sum_reference_global,
                      residual5_reference, stencil5, stencil5_rect, stencil5_reference, stencil5_residual,
                      stencil5_tb_held, stencil_box)
