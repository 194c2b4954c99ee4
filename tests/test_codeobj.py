"""Code-object guards on the built gfx950 library (host-only: reads the ELF
notes of the device code, runs nothing on a GPU).

* No kernel uses scratch.  A kernel whose unrolled arrays fall out of registers
  goes to scratch silently: round 3's VOP3-encoded logic pushed the replay
  kernel's burst loop past LLVM's full-unroll budget and its burst array to
  scratch, 2.4x its HBM traffic (the build now raises the threshold,
  __graft_entry__.HIP_FLAGS).
* The random rollout kernel fits 6 waves per SIMD (<= 85 VGPRs): the bench's
  two launches in flight sit side by side at 3 blocks per CU.
"""
import codeobj


# The one known exception (round 5): the eval-policy rollout kernels hold their
# current parent's record across its children (OTH_COOP_HOLD_EVAL), which fills
# their 128 VGPRs; hipcc spills a few per-batch values (<= 32 B, stored before
# the batch loop and reloaded once per batch, none in the ply or child loops).
# Measured (profiles/r05_notes.md): 3.810 ms per 1M-game launch against 3.945
# ms rereading the record per child, and 3.883 ms at 3 waves/SIMD without the
# spill.  Any other scratch, or more than this, fails.
# Round 6: the greedy kernels run at 5 waves per SIMD (<= 96 VGPRs), where hipcc
# spills a few per-batch values (the game index, the RNG increment, the opening
# boards; <= 68 B per lane, none in the child loop).  Measured against the
# same code at 4 waves without scratch (profiles/r06_notes.md, tools/
# gpu_greedy_ab.sh): 3.239e10 against 3.198e10 env-steps/s at two streams,
# 2.116 against 2.140 ms per one-stream launch; the scratch adds 16.8 MB of
# HBM writes per 1M-game launch (37.4 against 20.6 MB), 10 GB/s.
# rocprim's trampoline_kernel (four radix-sort instances, 48 B each) is library
# code in td_table.hip's bundle, not ours.
SCRATCH_ALLOWED = {"rollout_kernelILi2E": 32, "rollout_kernelILi1E": 68, "6detail17trampoline_kernel": 48}
# one kernel of each of the library's nine bundles (one per .hip file), in
# __graft_entry__.HIP_SRC's order: the guard below reads every one of them
ONE_PER_BUNDLE = ("14rollout_kernel", "15td_merge_kernel", "12solve_kernel", "13search_kernel", "11play_kernel",
                  "11task_kernel", "17split_solve_tasks", "19moves_expand_search", "20budget_deepen_kernel")


def test_no_kernel_uses_scratch():
    k = codeobj.kernels()
    names = " ".join(k)
    assert "rollout_kernel" in names and "replay_kernel" in names and "step_kernel" in names
    assert all(sub in names for sub in ONE_PER_BUNDLE), [sub for sub in ONE_PER_BUNDLE if sub not in names]
    spilled = {n: v["private_segment_fixed_size"] for n, v in k.items() if v.get("private_segment_fixed_size")}
    allowed = {n: b for n, b in spilled.items() if any(p in n and b <= cap for p, cap in SCRATCH_ALLOWED.items())}
    assert not set(spilled) - set(allowed), f"kernels with scratch: {spilled}"


def test_random_rollout_fits_six_waves():
    k = codeobj.kernels()
    rnd = [v for n, v in k.items() if "rollout_kernelILi0ELb0ELb0E" in n]
    assert len(rnd) == 1
    assert rnd[0]["vgpr_count"] <= 85, rnd[0]
