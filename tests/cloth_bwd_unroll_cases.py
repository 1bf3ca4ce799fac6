"""Shared by tests/test_cloth_bwd_unroll_bits_gpu.py and tools/record_cloth_adjoint_bits.py (--cases cloth_bwd_unroll_cases): substep
counts that tests/cloth_adjoint_bits_cases.py ((S, T) = (1, 1), (3, 2)) does not reach, chosen for a substep loop unrolled by two --
which cloth_fast_bwd.hip does not have today (round 9 built one, with the parent's bits, and it was slower: DESIGN.md 3.1), and which
the next attempt will.  Such a loop runs pairs and a tail, and the rollout's first substep (t = 0, s = 0, reversed last) has grasp
thresholds of its own:

    S = 2:  an even count, the first substep ends a pair;   S = 3:  one pair and an odd one;   S = 5:  the pair loop iterates

with T = 1 (only the macro step that holds the first substep) and T = 2 (a macro step after an odd tail, its records handed over across
the boundary), on a ragged body (65 particles: a second wave with one live lane) and a full one (512 = fold_cloth1's patch, P == Pp),
normalised and raw.  Inputs are cloth_adjoint_bits_cases.inputs' (per-macro-step cotangents on); one more case puts gripper 1 on a
particle."""
import cloth_adjoint_bits_cases as cc

GOLDEN = "cloth_bwd_unroll_bits.npz"
# (body, S, T, normalize, lists, two_grippers)
CASES = [(body, S, T, normalize, True, False) for body in ("rect5x13", "patch16x32") for S in (2, 3, 5) for T in (1, 2) for normalize in (True, False)]
CASES += [("patch16x32", 5, 2, True, True, True)]
case_id, run, inputs, oracle_forward = cc.case_id, cc.run, cc.inputs, cc.oracle_forward
