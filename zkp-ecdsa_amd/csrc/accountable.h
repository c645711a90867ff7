// Accountable attestations (include/zkattest.h: zk_accountable_*; k_accountable.hip, api_accountable.hip): one attestation and the escrow tag of its keyXcom
// as one "ZKC1" bundle.  The attestations, the key blinders, the keyXcom extractor and the tags are the existing pipelines'; what is declared here is the glue
// that keeps a window of bundles on the device between them.
#pragma once
#include "engine.h"
#include "accountable_plan.h"

// Prover.  One lane per bundle: key b = pk_xy[64 b .. 64 b + 32) into the tag prover's dense array
void launch_acc_keys(hipStream_t s, uint32_t n, const uint8_t* pk, uint8_t* key);
// One lane per bundle: its status (the attestation's, then the tag's), both part statuses where the caller wants them, the bundle's length (0 = empty slot)
void launch_acc_fold_prove(hipStream_t s, uint32_t n, const uint64_t* w_off, const int32_t* w_st, const int32_t* tag_st, int32_t* status, int32_t* part_status, uint64_t* len);
// Behind the scan of the lengths: the bundle's header at its final place, and the two records the byte mover (k_prove_rings.hip: k_pr_move) takes per bundle --
// record b = its attestation (at w_off[b] of its source), record n + b = its tag (at tag_stage + 472 b): join moves the two halves from two sources
void launch_acc_place(hipStream_t s, uint32_t n, const uint64_t* w_off, const uint64_t* len, uint64_t tag_stage, const uint64_t* out_off, uint8_t* out, uint64_t* rec_off,
                      uint64_t* rec_len, uint64_t* rec_dst);
// Verifier and split (tags == nullptr): one lane per bundle walks its headers (accountable_plan.h: zkc_walk): good[b], where its attestation lies and how long
// it is, where its tag lies, how long it is and where it goes (472 b) -- all lengths 0 in a bundle the walk refuses; status (nullptr: not wanted) = 0 or
// ZK_E_BAD_ENCODING.  Join (tags given): `bundles` holds the proofs, the walk is zkc_join_len's; a_src / a_len name the proof, t_src / t_len the tag in
// `tags`, a_len + t_len + 16 is the bundle's length where join accepts.
void launch_acc_walk(hipStream_t s, uint32_t n, const uint8_t* bundles, const uint64_t* bundle_off, const uint8_t* tags, const Wire& wire, uint8_t* good, uint64_t* a_src,
                     uint64_t* a_len, uint64_t* t_src, uint64_t* t_len, uint64_t* t_dst, uint64_t* len, int32_t* status);
// One lane per bundle folds (good, attestation, tag) into ok, status and first_bad (nullptr: not wanted)
void launch_acc_verdict(hipStream_t s, uint32_t n, const uint8_t* good, const uint8_t* a_ok, const int32_t* a_st, const uint8_t* t_ok, const int32_t* t_st, uint8_t* ok,
                        int32_t* status, uint32_t* first_bad);
// The `_rings` forms.  One lane per bundle: total[0] += its slot by accountable_plan.h's rule (zkc_capacity_rings), total[1] |= the entries of `R` the ids
// name (the caller zeroes both words and has checked zkc_capacity_fits)
void launch_acc_caps(hipStream_t s, uint32_t n, const uint32_t* ring_ids, const QuorumRings& R, uint64_t* total /*2*/);
// The open.  One lane per bundle merges the walk's refusal and the opener's id check with the opener's (status, ring, index) for the bundle's tag
void launch_acc_fold_open(hipStream_t s, uint32_t n, const uint8_t* good, const int32_t* o_st, const uint32_t* o_ring, const uint32_t* o_index, uint32_t* ring_out,
                          uint32_t* index, int32_t* status);

#if !defined(ZK_ACCOUNTABLE_KERNELS_ONLY)
#include "ctx.h"
// The internal paths of the tag calls, behind their argument checks (api_escrow.hip); the attestations', the blinders' and the keyXcoms' are quorum.h's
zk_status zkc_escrow_prove(zk_ctx* c, uint64_t B, const uint8_t* key, const uint8_t* com, const uint8_t* blinder, const zk_rng& rng, uint8_t* out, int32_t* status);   // zk_escrow_prove_batch_device
zk_status zkc_escrow_verify(zk_ctx* c, uint64_t B, const uint8_t* com, const uint8_t* tags, uint8_t* ok, int32_t* status);                                            // zk_escrow_verify_batch_device
zk_status zkc_rings_escrow_open(zk_ctx* c, uint64_t B, const uint8_t* secret, const uint8_t* tags, const uint32_t* ids, uint32_t* ring_out, uint32_t* index,
                                int32_t* status);                                                                                                                     // zk_rings_escrow_open_batch_device
#endif
