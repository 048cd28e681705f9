// dff_msm_table.h -- the problem table of the batched Markov-model calls: ONE 64-bit word per problem, slot << 11 | K_p.  K_p
// (<= 1024 < 2^11) is the problem's state count, `slot` says where its matrix lies: the problem's own index b for the estimator
// (dff_msm_batch.hip), the flux matrix for the Dirichlet solver (dff_msm_passage.hip), the transition matrix for propagation
// (dff_msm_propagate.hip).  The host packs (dff_an_markov.hip: MsmTable), the kernels unpack.  dff_sym_eig.hip reads bare
// counts: slot 0.
#pragma once

#define DFF_MSM_KBITS 11

__host__ inline long long msm_problem_pack(long long slot, int K) { return (slot << DFF_MSM_KBITS) | K; }
// of a word as the kernel holds it (64 bits, or the low 32 where slots stay below 2^20): the slot in d's own type, K_p an int
#define MSM_PROBLEM_SLOT(d) ((d) >> DFF_MSM_KBITS)
#define MSM_PROBLEM_K(d) ((int)((d) & ((1 << DFF_MSM_KBITS) - 1)))
