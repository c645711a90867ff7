/* Part of include/zkattest.h, which includes this file behind its own declarations: include zkattest.h, not this file.  It is a file of its own so that the
 * text of zkattest.h declares what it always did (its ZKC1 section is pinned word for word).
 *
 * ---- accountable attestations over several resident rings: one ring id per bundle, and the auditor's opening straight from bundles.  What the ZKC1 section of
 * zkattest.h lists as "not provided: one ring id per proof ... opening straight from bundles (split first)" is provided here: prove -> verify -> open for a
 * registry sharded over resident rings, one call per step, on ZKC1 bundles, with no active ring.  The calls are named zk_rings_accountable_*: the set of
 * zk_accountable_* names stays the nine of zkattest.h.  The wire format is ZKC1's, unchanged; no existing call changes.
 * Bundle b uses row b of msg_hash, sig, pk_xy, which, ring_ids, rng and rng_tags.  ring_ids[b] names a resident ring (zk_ctx_add_ring); the ACTIVE ring is
 * neither read nor changed, and a context with no active ring is not refused.
 * Buffer sizes: zk_rings_accountable_proof_max_size(ctx, ring_id) = 16 + zk_ring_proof_max_size(ctx, ring_id) + 472, and 0 for an id that is not resident or
 *   without params.
 * zk_rings_accountable_prove_batch: where bundle b succeeds its bytes are, byte for byte, the ZKC1 header, the proof zk_prove_batch_rings makes for row b with
 *   ring_ids[b], and the tag zk_escrow_prove_batch makes under row b of rng_tags with key = pk_xy[64 b : 64 b + 32], com = that proof's keyXcom and blinder =
 *   what zk_prove_key_blinders gives for row b -- in both protocol modes (in hardened mode each proof hashes its own ring's digest), both wire layouts and both
 *   RNG modes, whatever the comb width or build.  which[b] indexes the padded size of ring ring_ids[b].  per_proof_status is the first non-zero one of the
 *   attestation's zk_prove_batch_rings status (ZK_E_ARG for an id that is not resident), then the tag's; per_part_status (may be NULL) is filled as by
 *   zk_accountable_prove_batch.  A failed bundle gets an empty slot, the bundles behind it close up, no neighbour's byte changes.  When all ids name one ring,
 *   every output equals zk_accountable_prove_batch's with that ring active.
 *   Capacity: out_cap is decided exactly from the ids, before a byte of any output is written: ZK_E_BUFFER when out_cap < the sum over b of
 *   zk_rings_accountable_proof_max_size(ctx, ring_ids[b]) (a non-resident id contributes 0; a sum that passes 2^64 - 1 is refused, not wrapped).  The host form
 *   takes the sum on the host; the _device form with one small kernel and one read-back, which also yields the set of rings named: a window's staging follows
 *   the largest ring NAMED, not the largest resident.
 * zk_rings_accountable_verify_batch: the walk is zk_accountable_verify_batch's (ZK_E_BAD_ENCODING with ok 0 and first_bad 0) and needs no ring.  Otherwise the
 *   attestation is verified exactly as zk_verify_batch_rings verifies it with ring_ids[b] (zk_ctx_set_verify_level, zk_ctx_set_verify_reps, verifier_seeds row b
 *   or the library's own; ok 0 / ZK_E_ARG for an id that is not resident) and the tag exactly as zk_escrow_verify_batch does against the attestation's keyXcom.
 *   ok, per_proof_status and first_bad are folded by zk_accountable_verify_batch's rules; when all ids name one ring the result equals that call's with the ring
 *   active.
 * zk_rings_accountable_open_batch: the auditor's call on bundles.  Per bundle, in this order: ZK_E_ARG for an id that is neither resident nor
 *   ZK_ESCROW_RING_ANY, before the bundle's bytes are judged; ZK_E_BAD_ENCODING when the walk refuses the bundle, or for the tag's header, E1 or E2; otherwise 0.
 *   (ring_out, index) are exactly what zk_accountable_split_batch followed by zk_rings_escrow_open_batch gives on the same inputs: the lowest index, the factor
 *   4, ascending id order under ZK_ESCROW_RING_ANY, both outputs 0xFFFFFFFF where there is no match or under a non-zero status.  On the device only the tags are
 *   moved, 472 B per bundle: no attestation byte is copied anywhere (the host form uploads the bundles once, as the verifier does).  Call-level rules are
 *   zk_rings_escrow_open_batch's: ZK_E_BUFFER without params or an auditor key; ZK_E_OPENING, with nothing written, for a secret that is not the auditor
 *   key's; missing point indexes are built first.  OPENING DOES NOT VERIFY: a tag that zk_rings_accountable_verify_batch would refuse opens to whatever its
 *   E1, E2 decrypt to.  Verify first.
 * Call level, all three: ZK_E_BUFFER without params; the prover and the verifier also without an auditor key.  ZK_E_ARG for NULL pointers other than the
 *   optional arrays, for B >= 2^32 and while streamed jobs are queued.  B = 0 is ZK_OK with out_off[0] = 0.  The _device forms take every pointer, ring_ids and
 *   both rng->data included, in this context's HBM, 4-byte aligned, else ZK_E_ARG.  A call runs in windows of at most chunk x lanes bundles; what is
 *   witness-derived is zeroed by zk_ctx_wipe, zk_ctx_destroy and a failed call, as in the one-ring forms.  zk_last_timing reports the inner families plus
 *   "accountable_blinders", "accountable_layout", "accountable_walk", "accountable_verdict", and "accountable_caps" for the device prover's capacity kernel.
 * Not provided: threshold share calls on bundles (split first), tags inside ZKQ1 bundles, submit / wait, zk_pool_* and JSON forms, a caller-context binding.
 * Warning (2) of ZKL1 applies: rng_tags must be independent of rng.  DESIGN.md section 5h''''. */
#ifndef ZKATTEST_RINGS_ACCOUNTABLE_H
#define ZKATTEST_RINGS_ACCOUNTABLE_H
#ifndef ZKATTEST_H
#error "include zkattest.h"
#endif
uint64_t zk_rings_accountable_proof_max_size(const zk_ctx *ctx, uint32_t ring_id);   /* 0 where the id is not resident / without params */
zk_status zk_rings_accountable_prove_batch(zk_ctx *ctx, uint64_t B, const uint8_t *msg_hash /*Bx32*/, const uint8_t *sig /*Bx64*/, const uint8_t *pk_xy /*Bx64*/,
                                           const uint32_t *which /*B*/, const uint32_t *ring_ids /*B*/, const zk_rng *rng, const zk_rng *rng_tags, uint8_t *out,
                                           uint64_t out_cap, uint64_t *out_off /*B+1*/, int32_t *per_proof_status /*B*/, int32_t *per_part_status /*2B or NULL*/);
zk_status zk_rings_accountable_prove_batch_device(zk_ctx *ctx, uint64_t B, const void *d_msg_hash, const void *d_sig, const void *d_pk_xy, const void *d_which,
                                                  const void *d_ring_ids /*u32[B]*/, const zk_rng *rng_device, const zk_rng *rng_tags_device, void *d_out,
                                                  uint64_t out_cap, void *d_out_off /*u64[B+1]*/, void *d_per_proof_status /*i32[B]*/,
                                                  void *d_per_part_status /*i32[2B] or NULL*/);
zk_status zk_rings_accountable_verify_batch(zk_ctx *ctx, uint64_t B, const uint8_t *msg_hash /*Bx32*/, const uint8_t *bundles, const uint64_t *bundle_off /*B+1*/,
                                            const uint32_t *ring_ids /*B*/, const uint8_t *verifier_seeds /*Bx32 or NULL*/, uint8_t *ok /*B*/,
                                            int32_t *per_proof_status /*B*/, uint32_t *first_bad /*B or NULL*/);
zk_status zk_rings_accountable_verify_batch_device(zk_ctx *ctx, uint64_t B, const void *d_msg_hash, const void *d_bundles, const void *d_bundle_off /*u64[B+1]*/,
                                                   const void *d_ring_ids /*u32[B]*/, const void *d_verifier_seeds, void *d_ok, void *d_per_proof_status /*i32[B]*/,
                                                   void *d_first_bad /*u32[B] or NULL*/);
zk_status zk_rings_accountable_open_batch(zk_ctx *ctx, uint64_t B, const uint8_t secret_be32[32], const uint8_t *bundles, const uint64_t *bundle_off /*B+1*/,
                                          const uint32_t *ring_ids /*B; ZK_ESCROW_RING_ANY allowed*/, uint32_t *ring_out_u32 /*B*/, uint32_t *index_u32 /*B*/,
                                          int32_t *per_proof_status /*B*/);
zk_status zk_rings_accountable_open_batch_device(zk_ctx *ctx, uint64_t B, const void *d_secret_be32, const void *d_bundles, const void *d_bundle_off /*u64[B+1]*/,
                                                 const void *d_ring_ids /*u32[B]*/, void *d_ring_out_u32 /*u32[B]*/, void *d_index_u32 /*u32[B]*/,
                                                 void *d_per_proof_status /*i32[B]*/);
#endif
