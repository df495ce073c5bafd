// swimmer_kernels.hip -- the kernel families that have to be ONE translation unit, each in its own source file.
//
// Every family below reduces over a wave with __shfl_down, an ordinary (not force-inlined) function of the HIP
// headers that takes the reduction width as an argument.  The device compile of a translation unit sees all of its
// callers: where they all pass the same width the optimiser folds that constant into the function BEFORE it is
// inlined, and the shuffles' index arithmetic then comes out in another (equivalent, one instruction longer) form.
// The lane kernels' V2 moment rows reduce over 16 lanes (swimmer_rollout_lane.inc), everything else over 64, so the
// code of every kernel here depends on being compiled together with the lane kernels -- and theirs on the others.
// Compiled one by one, 137 of the library's 233 kernels change (profiles/r05_a_isa_kernel_diff.txt has the
// experiment), among them the riding covariance tile inside every n = 3 and row rollout kernel.  The files are
// self-contained (each compiles on its own, e.g. for a -S listing of its hot loops), but the library is built from
// this unit.  swimmer_abi.hip has no such tie and is a translation unit of its own.
#include "swimmer_rollout_row.hip"
#include "swimmer_rollout_n3.hip"
#include "swimmer_rollout_lane.hip"
#include "swimmer_rollout_safe_multi.hip"
#include "swimmer_step.hip"
#include "swimmer_cov.hip"
#include "swimmer_update.hip"
