"""Budget lists and helpers for height_pitch_eval_budgets_kernel (csrc/mvosr_hpeval_budgets.hip) — shared by
tests/test_hpeval_budgets_cases.py (CPU) and tests/test_gpu_hpeval_budgets.py (the device).  Test infrastructure.

The scenes are tests/hpeval_cases.py's; a budget list holds, per scene, the hypothesis numbers around which the best model or the
replay's state changes (the crafted first hypotheses, the spent samples, the tile's end at 512) and the ends of a 64-count replay
step.  The run at budget b of a (scene, case) is the scene's first b samples: its reference is
hpeval_cases.reference(..., positions[c][:b])."""
import numpy as np

import flat_cases as fc
import hpeval_cases as he

# scene -> budgets (the issue's table): 162 (scene, case, budget) combinations per model
BUDGETS = {
    "goal_late": (1, 7, 8, 9, 64, 511, 512, 513),
    "best_first_tile": (1, 3, 4, 5, 512, 513),
    "best_second_tile": (1, 3, 4, 5, 512, 513),
    "cases10": (1, 2, 31, 32, 33, 62, 63),
    "mix60": (1, 5, 63, 64, 65),
    "spent": (1, 2, 3, 4, 5, 6, 7, 12),
    "degenerate": (1, 2, 4),
    "neg": (1, 8, 64),
    "min12": (1, 16),
}
N_COMBINATIONS, N_RS_FEW = 324, 50      # both models; RS_FEW: none of the first b hypotheses has an inlier

# the outputs mvosr_height_pitch_eval_budgets_batch shares with mvosr_height_pitch_eval_batch, per (frame, case)
SHARED = ("ransac_height", "model", "best_ic", "used", "n_inliers", "refined_normal", "refined_pitch", "refined_mean", "refined_std",
          "height_t_mean", "sum_y", "sum_z", "status")
DOUBLES = ("ransac_height", "refined_pitch", "refined_mean", "refined_std", "height_t_mean", "sum_y", "sum_z")


def ref_at(model, s, c, budget):
    """The reference of scene s, case c at `budget` (computed once, shared by the tests)."""
    return he.ref_for(model, s, c, s.positions[c][:budget])


def carried_replay(state, counts, h0, M):
    """ransac_replay of csrc/mvosr_ransac.hpp on counts of hypotheses h0 .., its state (best, best_ic, used, done) carried:
    a strictly larger count replaces the best; the first new best above the goal stops the loop."""
    best, best_ic, used, done = state
    goal = float(M) * he.GOAL
    for t, c in enumerate(counts):
        if done:
            break
        if c > best_ic:
            best, best_ic = h0 + t, int(c)
            if c > goal:
                used, done = h0 + t + 1, True
    return best, best_ic, used, done


def cut_replay(counts, M, budgets, tile=he.TILE):
    """The budgets kernel's replay of `counts` (of the last budget's hypotheses): segments that end at a budget or at a tile's
    end, a snapshot at every budget -> [(best, best_ic, used)] per budget; `used` is the budget unless the stop came earlier."""
    cuts = sorted(set(budgets) | set(range(tile, budgets[-1], tile)) | {budgets[-1]})
    state, s, out = (-1, 0, budgets[-1], False), 0, {}
    for e in cuts:
        state = carried_replay(state, counts[s:e], s, M)
        if e in budgets:
            out[e] = (state[0], state[1], state[2] if state[3] else e)
        s = e
    return [out[b] for b in budgets]
