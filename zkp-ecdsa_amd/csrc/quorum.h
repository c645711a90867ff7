// Quorum proofs (include/zkattest.h: zk_quorum_*; k_quorum.hip, api_quorum.hip): k attestations and the k (k - 1) / 2 distinct-key proofs between their
// keyXcoms as one "ZKQ1" bundle.  The attestations, the key blinders, the keyXcom extractor and the distinct-key proofs are the existing pipelines'; what is
// declared here is the glue that keeps a window of whole quorums on the device between them.
#pragma once
#include "engine.h"
#include "quorum_plan.h"

struct QuorumShape {   // (a kernel argument) a window of nq whole quorums
    uint32_t nq, k, P;
};
// Prover.  One lane per (quorum, pair): key (pk_xy[0:32]), keyXcom and blinder of members i and j into the distinct prover's six arrays.
void launch_q_gather_prove(hipStream_t s, const QuorumShape& W, const uint8_t* pk, const uint8_t* com, const uint8_t* blinder, uint8_t* key1, uint8_t* com1, uint8_t* blinder1,
                           uint8_t* key2, uint8_t* com2, uint8_t* blinder2);
// One lane per quorum: its status (members, then equal keys, then pairs), the members' statuses where the caller wants them, the bundle's length (0 = empty slot)
void launch_q_fold_prove(hipStream_t s, const QuorumShape& W, const uint64_t* w_off, const int32_t* w_st, const int32_t* pair_st, int32_t* q_status, int32_t* member_status,
                         uint64_t* len);
// Behind the scan of the lengths: the bundle's header at its final place, and the two records the byte mover (k_prove_rings.hip: k_pr_move) takes per quorum
void launch_q_place(hipStream_t s, const QuorumShape& W, const uint64_t* w_off, const uint64_t* len, uint64_t pair_stage, const uint64_t* out_off, uint8_t* out, uint64_t* rec_off,
                    uint64_t* rec_len, uint64_t* rec_dst);
// Verifier.  One lane per quorum walks the bundle's headers (quorum_plan.h: zkq_walk): good[q], and per member where it lies and how long it is (0 in a bundle
// the walk refuses); per quorum where its pairs' proofs lie and where they go in the staging area.
void launch_q_walk(hipStream_t s, const QuorumShape& W, const uint8_t* bundles, const uint64_t* bundle_off, const Wire& wire, uint8_t* good, uint64_t* walk /*nq (k + 1)*/,
                   uint64_t* m_src, uint64_t* m_len, uint64_t* p_src, uint64_t* p_len, uint64_t* p_dst);
// One lane per (quorum, pair): the keyXcoms of members i and j, in that direction
void launch_q_gather_verify(hipStream_t s, const QuorumShape& W, const uint8_t* com, uint8_t* com1, uint8_t* com2);
// One lane per quorum folds its k + P (ok, status) pairs into ok, status and first_bad (nullptr: not wanted)
void launch_q_verdict(hipStream_t s, const QuorumShape& W, const uint8_t* good, const uint8_t* m_ok, const int32_t* m_st, const uint8_t* p_ok, const int32_t* p_st, uint8_t* ok,
                      int32_t* status, uint32_t* first_bad);
// The `_rings` forms.  One lane per quorum: caps[q] = its slot's capacity by quorum_plan.h's rule; total[0] += the capacities, total[1] |= the entries of `R` the
// ids name (the caller zeroes both words).
void launch_q_caps(hipStream_t s, uint32_t Q, uint32_t k, const uint32_t* ring_ids, const QuorumRings& R, uint64_t* caps, uint64_t* total /*2*/);

#if !defined(ZK_QUORUM_KERNELS_ONLY)
#include "ctx.h"
// The `_rings` forms (api_quorum.hip; api_accountable.hip's share them): the context's rings as the capacity rules see them, and the largest proof among the
// entries of the bit set `used`
void quorum_rings_table(const zk_ctx* c, QuorumRings& R);
uint64_t quorum_largest(const QuorumRings& R, uint32_t used);
// The internal paths of the existing calls, behind their argument checks (each in the file of its call)
zk_status zkq_prove_members(zk_ctx* c, uint64_t B, const uint8_t* d_msg, const uint8_t* d_sig, const uint8_t* d_pk, const uint32_t* d_which, const zk_rng& rng, uint8_t* d_out,
                            uint64_t out_cap, uint64_t* d_out_off, int32_t* d_status);                                                                  // api.hip: zk_prove_batch_device
zk_status zkq_verify_members(zk_ctx* c, uint64_t B, const uint8_t* d_msg, const uint8_t* d_proofs, const uint64_t* d_off, const uint8_t* d_vseeds, uint8_t* d_ok,
                             int32_t* d_status);                                                                                                        // api_verify.hip: zk_verify_batch_device
zk_status zkq_prove_members_rings(zk_ctx* c, uint64_t B, const uint8_t* d_msg, const uint8_t* d_sig, const uint8_t* d_pk, const uint32_t* d_which, const uint32_t* d_ids,
                                  const zk_rng& rng, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off, int32_t* d_status);                         // api.hip: zk_prove_batch_rings_device
zk_status zkq_verify_members_rings(zk_ctx* c, uint64_t B, const uint8_t* d_msg, const uint8_t* d_proofs, const uint64_t* d_off, const uint32_t* d_ids, const uint8_t* d_vseeds,
                                   uint8_t* d_ok, int32_t* d_status);                                                                                   // api_verify.hip: zk_verify_batch_rings_device
zk_status zkq_key_blinders(zk_ctx* c, uint64_t B, const zk_rng& rng, uint8_t* d_out);                                                                   // api_rering.hip: zk_prove_key_blinders_device
zk_status zkq_distinct_prove(zk_ctx* c, uint64_t B, const uint8_t* key1, const uint8_t* com1, const uint8_t* blinder1, const uint8_t* key2, const uint8_t* com2,
                             const uint8_t* blinder2, const zk_rng& rng, uint8_t* out, int32_t* status);                                                // api_distinct.hip: zk_distinct_prove_batch_device
zk_status zkq_distinct_verify(zk_ctx* c, uint64_t B, const uint8_t* com1, const uint8_t* com2, const uint8_t* proofs, uint8_t* ok, int32_t* status);   // api_distinct.hip: zk_distinct_verify_batch_device
#endif
