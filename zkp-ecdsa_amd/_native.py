"""ctypes binding of libzkattest_hip.so (C ABI: include/zkattest.h).  Fails loudly when the library is missing:
there is no CPU fallback in the product path."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZKATTEST_LIB selects another build of the same library (e.g. a different comb width, csrc/Makefile TOM_WIN_BITS)
LIB_PATH = os.environ.get('ZKATTEST_LIB') or os.path.join(_HERE, 'lib', 'libzkattest_hip.so')
CSRC = os.path.join(_HERE, 'csrc')

# every symbol include/zkattest.h declares
SYMBOLS = [
    'zk_ctx_create', 'zk_ctx_destroy', 'zk_strerror', 'zk_last_error', 'zk_ctx_set_params', 'zk_ctx_set_ring',
    'zk_ctx_set_ring_device', 'zk_ctx_wipe', 'zk_last_wall_ms', 'zk_ctx_set_timing', 'zk_keys_to_ints', 'zk_ctx_set_chunk', 'zk_ctx_set_lanes', 'zk_ctx_set_comb_bits', 'zk_ctx_set_batch_verify', 'zk_proof_max_size', 'zk_prove_batch', 'zk_prove_batch_device',
    'zk_verify_batch', 'zk_verify_batch_device', 'zk_synth_workload', 'zk_synth_params', 'zk_last_timing',
    'zk_proof_to_json', 'zk_proof_from_json', 'zk_host_alloc', 'zk_host_free', 'zk_ctx_set_host_taper', 'zk_ctx_set_slice', 'zk_ctx_set_mode', 'zk_ring_digest', 'zk_hardened_h',
    'zk_pool_create', 'zk_pool_destroy', 'zk_pool_size', 'zk_pool_ctx', 'zk_pool_last_error', 'zk_pool_ring_transport', 'zk_pool_rccl_library', 'zk_pool_shard',
    'zk_pool_set_params', 'zk_pool_set_ring', 'zk_pool_prove_batch', 'zk_pool_verify_batch',
    'zk_pool_host_alloc', 'zk_pool_host_free', 'zk_pool_numa_node', 'zk_pool_test_locality', 'zk_pool_shard_ms', 'zk_ctx_copy_probe', 'zk_ctx_set_wire', 'zk_proof_pack', 'zk_proof_unpack', 'zk_pool_prove_batch_device', 'zk_pool_device_alloc', 'zk_pool_device_free',
    'zk_prove_submit', 'zk_prove_submit_device', 'zk_prove_wait', 'zk_verify_submit', 'zk_verify_wait', 'zk_test_counter', 'zk_test_tom_commit_shape', 'zk_ctx_set_key_tables',
    'zk_proofs_to_json_batch', 'zk_proofs_from_json_batch', 'zk_ctx_set_ring_fold',
    'zk_pool_prove_submit', 'zk_pool_prove_wait', 'zk_pool_verify_submit', 'zk_pool_verify_wait', 'zk_ctx_set_verify_groups',
    'zk_ctx_set_verify_level', 'zk_pool_set_verify_level', 'zk_ctx_set_verify_reps', 'zk_pool_set_verify_reps',
    'zk_ctx_add_ring', 'zk_ctx_add_ring_device', 'zk_ctx_use_ring', 'zk_ctx_drop_ring', 'zk_ring_info', 'zk_verify_batch_rings', 'zk_verify_batch_rings_device',
    'zk_pool_add_ring', 'zk_pool_use_ring', 'zk_pool_drop_ring', 'zk_pool_verify_batch_rings',
    'zk_ctx_update_ring', 'zk_pool_update_ring',
    'zk_prove_batch_rings', 'zk_prove_batch_rings_device', 'zk_pool_prove_batch_rings', 'zk_ring_proof_max_size',
    'zk_screen_batch', 'zk_screen_batch_device', 'zk_screen_batch_rings', 'zk_screen_batch_rings_device',
    'zk_recover_batch', 'zk_recover_batch_device', 'zk_recover_batch_rings', 'zk_recover_batch_rings_device',
    'zk_member_proof_size', 'zk_member_prove_batch', 'zk_member_prove_batch_device', 'zk_member_verify_batch', 'zk_member_verify_batch_device',
    'zk_member_proof_size_ring', 'zk_member_prove_batch_rings', 'zk_member_prove_batch_rings_device', 'zk_member_verify_batch_rings', 'zk_member_verify_batch_rings_device',
    'zk_member_prove_batch_bound', 'zk_member_prove_batch_bound_device', 'zk_member_verify_batch_bound', 'zk_member_verify_batch_bound_device',
    'zk_member_prove_batch_rings_bound', 'zk_member_prove_batch_rings_bound_device', 'zk_member_verify_batch_rings_bound', 'zk_member_verify_batch_rings_bound_device',
    'zk_prove_key_blinders', 'zk_prove_key_blinders_device', 'zk_proof_rering_batch', 'zk_proof_rering_batch_device',
    'zk_proof_rering_batch_rings', 'zk_proof_rering_batch_rings_device',
    'zk_link_proof_size', 'zk_link_prove_batch', 'zk_link_prove_batch_device', 'zk_link_verify_batch', 'zk_link_verify_batch_device',
    'zk_proof_key_commitments', 'zk_proof_key_commitments_device',
    'zk_distinct_proof_size', 'zk_distinct_prove_batch', 'zk_distinct_prove_batch_device', 'zk_distinct_verify_batch', 'zk_distinct_verify_batch_device',
    'zk_quorum_pair_count', 'zk_quorum_proof_max_size', 'zk_quorum_prove_batch', 'zk_quorum_prove_batch_device', 'zk_quorum_verify_batch', 'zk_quorum_verify_batch_device',
    'zk_rings_quorum_proof_max_size', 'zk_rings_quorum_prove_batch', 'zk_rings_quorum_prove_batch_device', 'zk_rings_quorum_verify_batch', 'zk_rings_quorum_verify_batch_device',
    'zk_ctx_set_auditor', 'zk_escrow_keygen', 'zk_escrow_tag_size', 'zk_escrow_prove_batch', 'zk_escrow_prove_batch_device', 'zk_escrow_verify_batch',
    'zk_escrow_verify_batch_device', 'zk_escrow_open_batch', 'zk_escrow_open_batch_device',
    'zk_rings_escrow_open_batch', 'zk_rings_escrow_open_batch_device',
    'zk_auditors_share_size', 'zk_auditors_split_key', 'zk_ctx_set_auditors', 'zk_auditors_share_batch', 'zk_auditors_share_batch_device',
    'zk_auditors_share_verify_batch', 'zk_auditors_share_verify_batch_device', 'zk_auditors_combine_batch', 'zk_auditors_combine_batch_device',
    'zk_accountable_proof_max_size', 'zk_accountable_prove_batch', 'zk_accountable_prove_batch_device', 'zk_accountable_verify_batch',
    'zk_accountable_verify_batch_device', 'zk_accountable_split_batch', 'zk_accountable_split_batch_device', 'zk_accountable_join_batch',
    'zk_accountable_join_batch_device',
    'zk_test_field_op', 'zk_test_tom_commit', 'zk_test_p256_fixed_mul', 'zk_test_sha256', 'zk_test_rng_draws', 'zk_test_exp_sum',
    'zk_test_msm_sum', 'zk_test_pmsm_sum',
]
# ... and what include/zkattest_rings_accountable.h, the part of it that is a file of its own, declares
RINGS_ACCOUNTABLE_SYMBOLS = [
    'zk_rings_accountable_proof_max_size', 'zk_rings_accountable_prove_batch', 'zk_rings_accountable_prove_batch_device', 'zk_rings_accountable_verify_batch',
    'zk_rings_accountable_verify_batch_device', 'zk_rings_accountable_open_batch', 'zk_rings_accountable_open_batch_device',
]

STATUS_TEXT = {
    0: 'ok', 1: 'point not in group', 2: 'invalid public key', 3: 'T[i] is at infinity', 4: 'T1 is at infinity',
    5: 'P/Q/R is at infinity', 6: "Points don't add up!", 7: 'R is at infinity', 8: 'params not found',
    9: 'security level not achieved', 10: 'error deserializing', 11: 'randomness stream exhausted',
    12: 'buffer too small or context not configured', 13: 'incorrect interpolation', 14: 'invalid argument',
    15: 'HIP runtime failure', 16: "the index and blinder do not open the proof's key commitment",   # (link proofs: the key and a blinder do not open com1 / com2)
}
E_OPENING = 16


def _ring_changes(changes):
    """changes: a dict {index: key_bytes} or a list of (index, key_bytes), applied in order -> (count, u64 array or None, key bytes or None)"""
    items = list(changes.items()) if isinstance(changes, dict) else list(changes)
    if not items:
        return 0, None, None
    for _, k in items:
        if len(k) != 32:
            raise ValueError('a ring key is 32 bytes')
    return len(items), (C.c_uint64 * len(items))(*[int(i) for i, _ in items]), b''.join(bytes(k) for _, k in items)


class ZkRng(C.Structure):
    _fields_ = [('mode', C.c_int32), ('data', C.c_void_p), ('stride_blocks', C.c_uint64)]


def build(jobs=8):
    """Compile the HIP library for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(['make', '-C', CSRC, '-j%d' % jobs, '-s'])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError('libzkattest_hip.so is not built (run __graft_entry__.build()); the engine has no CPU fallback')
        L = C.CDLL(LIB_PATH)
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.zk_ctx_create.argtypes = [i32, C.POINTER(vp)]
        L.zk_ctx_destroy.argtypes = [vp]
        L.zk_ctx_destroy.restype = None
        L.zk_strerror.argtypes = [i32]
        L.zk_strerror.restype = C.c_char_p
        L.zk_last_error.argtypes = [vp]
        L.zk_last_error.restype = C.c_char_p
        L.zk_ctx_set_params.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, u32]
        L.zk_ctx_set_ring.argtypes = [vp, C.c_char_p, u64]
        L.zk_ctx_set_ring_device.argtypes = [vp, vp, u64]
        L.zk_keys_to_ints.argtypes = [vp, u64, C.c_char_p, vp, vp]
        L.zk_ctx_set_chunk.argtypes = [vp, u32]
        L.zk_ctx_set_lanes.argtypes = [vp, u32]
        L.zk_ctx_set_comb_bits.argtypes = [vp, u32]
        L.zk_ctx_set_batch_verify.argtypes = [vp, u32]
        L.zk_proof_max_size.argtypes = [vp]
        L.zk_proof_max_size.restype = u64
        L.zk_prove_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, vp, C.POINTER(ZkRng), vp, u64, vp, vp]
        L.zk_prove_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, C.POINTER(ZkRng), vp, u64, vp, vp]
        L.zk_verify_batch.argtypes = [vp, u64, C.c_char_p, vp, vp, C.c_char_p, vp, vp]
        L.zk_host_alloc.argtypes = [C.c_size_t]
        L.zk_host_alloc.restype = vp
        L.zk_host_free.argtypes = [vp]
        L.zk_host_free.restype = None
        L.zk_verify_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]
        L.zk_synth_workload.argtypes = [vp, u64, u64, u64, vp, vp, vp, vp, vp, vp]
        L.zk_synth_params.argtypes = [vp, u64, vp, vp, vp]
        L.zk_last_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.POINTER(C.c_float), u32]
        L.zk_last_timing.restype = u32
        L.zk_proof_to_json.argtypes = [C.c_char_p, u64, vp, u64, C.POINTER(u64)]
        L.zk_proof_from_json.argtypes = [C.c_char_p, u64, vp, u64, C.POINTER(u64)]
        L.zk_ctx_set_host_taper.argtypes = [vp, u32]
        L.zk_ctx_set_slice.argtypes = [vp, u32]
        L.zk_ctx_set_mode.argtypes = [vp, u32]
        L.zk_ctx_set_verify_level.argtypes = [vp, u32]
        L.zk_pool_set_verify_level.argtypes = [vp, u32]
        L.zk_ctx_set_verify_reps.argtypes = [vp, u32]
        L.zk_pool_set_verify_reps.argtypes = [vp, u32]
        L.zk_ctx_add_ring.argtypes = [vp, C.c_char_p, u64, C.POINTER(u32)]
        L.zk_ctx_add_ring_device.argtypes = [vp, vp, u64, C.POINTER(u32)]
        L.zk_ctx_use_ring.argtypes = [vp, u32]
        L.zk_ctx_drop_ring.argtypes = [vp, u32]
        L.zk_ring_info.argtypes = [vp, u32, C.POINTER(u64), C.POINTER(u32), C.POINTER(u32), C.POINTER(u64)]
        L.zk_verify_batch_rings.argtypes = [vp, u64, C.c_char_p, vp, vp, vp, C.c_char_p, vp, vp]
        L.zk_verify_batch_rings_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
        L.zk_pool_add_ring.argtypes = [vp, C.c_char_p, u64, C.POINTER(u32)]
        L.zk_pool_use_ring.argtypes = [vp, u32]
        L.zk_ctx_update_ring.argtypes = [vp, u32, u64, vp, C.c_char_p, u64]
        L.zk_pool_update_ring.argtypes = [vp, u32, u64, vp, C.c_char_p, u64]
        L.zk_pool_drop_ring.argtypes = [vp, u32]
        L.zk_pool_verify_batch_rings.argtypes = [vp, u64, C.c_char_p, vp, vp, vp, vp, C.c_char_p, vp, vp]
        L.zk_prove_batch_rings.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, vp, vp, C.POINTER(ZkRng), vp, u64, vp, vp]
        L.zk_prove_batch_rings_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, C.POINTER(ZkRng), vp, u64, vp, vp]
        L.zk_pool_prove_batch_rings.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, vp, vp, C.POINTER(ZkRng), vp, u64, vp, vp, vp]
        L.zk_ring_proof_max_size.argtypes = [vp, u32]
        L.zk_screen_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, vp, vp, vp]
        L.zk_screen_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]
        L.zk_screen_batch_rings.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, vp, vp, vp, vp]
        L.zk_screen_batch_rings_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
        L.zk_recover_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, vp, vp, vp]
        L.zk_recover_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, vp]
        L.zk_recover_batch_rings.argtypes = [vp, u64, C.c_char_p, C.c_char_p, vp, vp, vp, vp]
        L.zk_recover_batch_rings_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]
        L.zk_ring_proof_max_size.restype = u64
        L.zk_member_proof_size.argtypes = [vp]
        L.zk_member_proof_size.restype = u64
        L.zk_member_prove_batch.argtypes = [vp, u64, vp, C.c_char_p, C.POINTER(ZkRng), vp, vp, vp, u64, vp]
        L.zk_member_prove_batch_device.argtypes = [vp, u64, vp, vp, C.POINTER(ZkRng), vp, vp, vp, u64, vp]
        L.zk_member_verify_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, vp, vp]
        L.zk_member_verify_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, vp]
        L.zk_member_proof_size_ring.argtypes = [vp, C.c_uint32]
        L.zk_member_proof_size_ring.restype = u64
        L.zk_member_prove_batch_rings.argtypes = [vp, u64, vp, vp, C.c_char_p, C.POINTER(ZkRng), vp, vp, vp, u64, vp, vp]
        L.zk_member_prove_batch_rings_device.argtypes = [vp, u64, vp, vp, vp, C.POINTER(ZkRng), vp, vp, vp, u64, vp, vp]
        L.zk_member_verify_batch_rings.argtypes = [vp, u64, C.c_char_p, C.c_char_p, vp, vp, C.c_char_p, vp, vp]
        L.zk_member_verify_batch_rings_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
        # the bound forms ("ZKMB"): 32 context bytes per proof after `which` (prove) / after the commitments (verify)
        L.zk_member_prove_batch_bound.argtypes = [vp, u64, vp, C.c_char_p, C.c_char_p, C.POINTER(ZkRng), vp, vp, vp, u64, vp]
        L.zk_member_prove_batch_bound_device.argtypes = [vp, u64, vp, vp, vp, C.POINTER(ZkRng), vp, vp, vp, u64, vp]
        L.zk_member_verify_batch_bound.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, vp, vp]
        L.zk_member_verify_batch_bound_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]
        L.zk_member_prove_batch_rings_bound.argtypes = [vp, u64, vp, C.c_char_p, vp, C.c_char_p, C.POINTER(ZkRng), vp, vp, vp, u64, vp, vp]
        L.zk_member_prove_batch_rings_bound_device.argtypes = [vp, u64, vp, vp, vp, vp, C.POINTER(ZkRng), vp, vp, vp, u64, vp, vp]
        L.zk_member_verify_batch_rings_bound.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, vp, vp, C.c_char_p, vp, vp]
        L.zk_member_verify_batch_rings_bound_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]
        # re-ring: keyXcom's blinders, and a proof's GKProof section replaced by one for the active ring
        L.zk_prove_key_blinders.argtypes = [vp, u64, C.POINTER(ZkRng), vp]
        L.zk_prove_key_blinders_device.argtypes = [vp, u64, C.POINTER(ZkRng), vp]
        L.zk_proof_rering_batch.argtypes = [vp, u64, C.c_char_p, vp, vp, vp, C.c_char_p, C.POINTER(ZkRng), vp, u64, vp, vp]
        L.zk_proof_rering_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, C.POINTER(ZkRng), vp, u64, vp, vp]
        L.zk_proof_rering_batch_rings.argtypes = [vp, u64, C.c_char_p, vp, vp, vp, vp, C.c_char_p, C.POINTER(ZkRng), vp, u64, vp, vp]
        L.zk_proof_rering_batch_rings_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, C.POINTER(ZkRng), vp, u64, vp, vp]
        # link proofs ("ZKL1"): two commitments hide the same key; keyXcom of ZKA1 / ZK1P proofs
        L.zk_link_proof_size.argtypes = []
        L.zk_link_proof_size.restype = u64
        L.zk_link_prove_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(ZkRng), vp, u64, vp]
        L.zk_link_prove_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, C.POINTER(ZkRng), vp, u64, vp]
        L.zk_link_verify_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, vp, vp]
        L.zk_link_verify_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, vp]
        # distinct-key proofs ("ZKD1"): two commitments hide different keys
        L.zk_distinct_proof_size.argtypes = []
        L.zk_distinct_proof_size.restype = u64
        L.zk_distinct_prove_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(ZkRng), vp, u64, vp]
        L.zk_distinct_prove_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, C.POINTER(ZkRng), vp, u64, vp]
        L.zk_distinct_verify_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, vp, vp]
        L.zk_distinct_verify_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, vp]
        # quorum proofs ("ZKQ1"): k attestations and the distinct-key proofs between their keyXcoms as one bundle
        L.zk_quorum_pair_count.argtypes = [C.c_uint32]
        L.zk_quorum_pair_count.restype = u64
        L.zk_quorum_proof_max_size.argtypes = [vp, C.c_uint32]
        L.zk_quorum_proof_max_size.restype = u64
        L.zk_quorum_prove_batch.argtypes = [vp, u64, C.c_uint32, C.c_char_p, C.c_char_p, C.c_char_p, vp, C.POINTER(ZkRng), C.POINTER(ZkRng), vp, u64, vp, vp, vp]
        L.zk_quorum_prove_batch_device.argtypes = [vp, u64, C.c_uint32, vp, vp, vp, vp, C.POINTER(ZkRng), C.POINTER(ZkRng), vp, u64, vp, vp, vp]
        L.zk_quorum_verify_batch.argtypes = [vp, u64, C.c_uint32, C.c_char_p, C.c_char_p, vp, C.c_char_p, vp, vp, vp]
        L.zk_quorum_verify_batch_device.argtypes = [vp, u64, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]
        # ... with one resident ring id per member
        L.zk_rings_quorum_proof_max_size.argtypes = [vp, C.c_uint32, vp]
        L.zk_rings_quorum_proof_max_size.restype = u64
        L.zk_rings_quorum_prove_batch.argtypes = [vp, u64, C.c_uint32, C.c_char_p, C.c_char_p, C.c_char_p, vp, vp, C.POINTER(ZkRng), C.POINTER(ZkRng), vp, u64, vp, vp, vp]
        L.zk_rings_quorum_prove_batch_device.argtypes = [vp, u64, C.c_uint32, vp, vp, vp, vp, vp, C.POINTER(ZkRng), C.POINTER(ZkRng), vp, u64, vp, vp, vp]
        L.zk_rings_quorum_verify_batch.argtypes = [vp, u64, C.c_uint32, C.c_char_p, C.c_char_p, vp, vp, C.c_char_p, vp, vp, vp]
        L.zk_rings_quorum_verify_batch_device.argtypes = [vp, u64, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp]
        # escrow tags ("ZKT1"): ElGamal of a committed key under an auditor's key, and the auditor's opening
        L.zk_ctx_set_auditor.argtypes = [vp, C.c_char_p]
        L.zk_escrow_keygen.argtypes = [vp, C.c_char_p, vp]
        L.zk_escrow_tag_size.argtypes = []
        L.zk_escrow_tag_size.restype = u64
        L.zk_escrow_prove_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(ZkRng), vp, u64, vp]
        L.zk_escrow_prove_batch_device.argtypes = [vp, u64, vp, vp, vp, C.POINTER(ZkRng), vp, u64, vp]
        L.zk_escrow_verify_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, vp, vp]
        L.zk_escrow_verify_batch_device.argtypes = [vp, u64, vp, vp, vp, vp]
        L.zk_escrow_open_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, vp, vp]
        L.zk_escrow_open_batch_device.argtypes = [vp, u64, vp, vp, vp, vp]
        # ... against any resident ring, through the rings' resident point indexes: one ring id per tag
        L.zk_rings_escrow_open_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, vp, vp, vp, vp]
        L.zk_rings_escrow_open_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]
        # threshold opening ("ZKS1"): t of n auditors open a tag through verifiable shares
        L.zk_auditors_share_size.argtypes = []
        L.zk_auditors_share_size.restype = u64
        L.zk_auditors_split_key.argtypes = [vp, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(ZkRng), vp, vp]
        L.zk_ctx_set_auditors.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_char_p]
        L.zk_auditors_share_batch.argtypes = [vp, u64, C.c_uint32, C.c_char_p, C.c_char_p, C.POINTER(ZkRng), vp, u64, vp]
        L.zk_auditors_share_batch_device.argtypes = [vp, u64, C.c_uint32, vp, vp, C.POINTER(ZkRng), vp, u64, vp]
        L.zk_auditors_share_verify_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, vp, vp]
        L.zk_auditors_share_verify_batch_device.argtypes = [vp, u64, vp, vp, vp, vp]
        L.zk_auditors_combine_batch.argtypes = [vp, u64, C.c_uint32, vp, C.c_char_p, C.c_char_p, vp, vp, vp, vp]
        L.zk_auditors_combine_batch_device.argtypes = [vp, u64, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]
        # accountable attestations ("ZKC1"): an attestation and the escrow tag of its keyXcom as one bundle
        L.zk_accountable_proof_max_size.argtypes = [vp]
        L.zk_accountable_proof_max_size.restype = u64
        L.zk_accountable_prove_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, vp, C.POINTER(ZkRng), C.POINTER(ZkRng), vp, u64, vp, vp, vp]
        L.zk_accountable_prove_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, C.POINTER(ZkRng), C.POINTER(ZkRng), vp, u64, vp, vp, vp]
        L.zk_accountable_verify_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, vp, C.c_char_p, vp, vp, vp]
        L.zk_accountable_verify_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
        L.zk_accountable_split_batch.argtypes = [vp, u64, C.c_char_p, vp, vp, u64, vp, vp, vp]
        L.zk_accountable_split_batch_device.argtypes = [vp, u64, vp, vp, vp, u64, vp, vp, vp]
        L.zk_accountable_join_batch.argtypes = [vp, u64, C.c_char_p, vp, C.c_char_p, vp, u64, vp, vp]
        L.zk_accountable_join_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, u64, vp, vp]
        # ... over several rings: one resident ring id per bundle, and the auditor's opening straight from bundles
        L.zk_rings_accountable_proof_max_size.argtypes = [vp, u32]
        L.zk_rings_accountable_proof_max_size.restype = u64
        L.zk_rings_accountable_prove_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, vp, vp, C.POINTER(ZkRng), C.POINTER(ZkRng), vp, u64, vp, vp, vp]
        L.zk_rings_accountable_prove_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, C.POINTER(ZkRng), C.POINTER(ZkRng), vp, u64, vp, vp, vp]
        L.zk_rings_accountable_verify_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, vp, vp, C.c_char_p, vp, vp, vp]
        L.zk_rings_accountable_verify_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]
        L.zk_rings_accountable_open_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, vp, vp, vp, vp, vp]
        L.zk_rings_accountable_open_batch_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp]
        L.zk_proof_key_commitments.argtypes = [vp, u64, C.c_char_p, vp, vp, vp]
        L.zk_proof_key_commitments_device.argtypes = [vp, u64, vp, vp, vp, vp]
        L.zk_ring_digest.argtypes = [vp, vp]
        L.zk_hardened_h.argtypes = [C.c_char_p, u64, vp, vp]
        L.zk_pool_create.argtypes = [C.POINTER(C.c_int), i32, C.POINTER(vp)]
        L.zk_pool_destroy.argtypes = [vp]
        L.zk_pool_destroy.restype = None
        L.zk_pool_size.argtypes = [vp]
        L.zk_pool_ctx.argtypes = [vp, i32]
        L.zk_pool_ctx.restype = vp
        L.zk_pool_last_error.argtypes = [vp]
        L.zk_pool_last_error.restype = C.c_char_p
        L.zk_pool_ring_transport.argtypes = [vp]
        L.zk_pool_ring_transport.restype = C.c_char_p
        L.zk_pool_rccl_library.argtypes = [vp]
        L.zk_pool_rccl_library.restype = C.c_char_p
        L.zk_pool_shard.argtypes = [vp, u64, i32, C.POINTER(u64), C.POINTER(u64)]
        L.zk_pool_shard.restype = None
        L.zk_pool_set_params.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, u32]
        L.zk_pool_set_ring.argtypes = [vp, C.c_char_p, u64]
        L.zk_pool_prove_batch.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, vp, C.POINTER(ZkRng), vp, u64, vp, vp, vp]
        L.zk_pool_verify_batch.argtypes = [vp, u64, C.c_char_p, vp, vp, vp, C.c_char_p, vp, vp]
        L.zk_proofs_to_json_batch.argtypes = [u64, vp, vp, vp, u64, vp, vp, u32]
        L.zk_proofs_from_json_batch.argtypes = [u64, vp, vp, vp, u64, vp, vp, u32]
        L.zk_prove_submit.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, vp, C.POINTER(ZkRng), vp, u64, vp, vp, C.POINTER(vp)]
        L.zk_prove_submit_device.argtypes = [vp, u64, vp, vp, vp, vp, C.POINTER(ZkRng), vp, u64, vp, vp, C.POINTER(vp)]
        L.zk_prove_wait.argtypes = [vp, vp]
        L.zk_verify_submit.argtypes = [vp, u64, C.c_char_p, vp, vp, C.c_char_p, vp, vp, C.POINTER(vp)]
        L.zk_verify_wait.argtypes = [vp, vp]
        L.zk_ctx_set_ring_fold.argtypes = [vp, u32]
        L.zk_ctx_set_key_tables.argtypes = [vp, u32]
        L.zk_ctx_set_verify_groups.argtypes = [vp, u32]
        L.zk_test_counter.argtypes = [vp, i32]
        L.zk_test_counter.restype = u64
        L.zk_pool_prove_submit.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, vp, C.POINTER(ZkRng), vp, u64, vp, vp, vp, C.POINTER(vp)]
        L.zk_pool_prove_wait.argtypes = [vp, vp]
        L.zk_pool_verify_submit.argtypes = [vp, u64, C.c_char_p, vp, vp, vp, C.c_char_p, vp, vp, C.POINTER(vp)]
        L.zk_pool_verify_wait.argtypes = [vp, vp]
        L.zk_pool_prove_batch_device.argtypes = [vp, u64, C.c_char_p, C.c_char_p, C.c_char_p, vp, C.POINTER(ZkRng), vp, vp, vp, vp, vp]
        L.zk_pool_device_alloc.argtypes = [vp, i32, C.c_size_t]
        L.zk_pool_device_alloc.restype = vp
        L.zk_pool_device_free.argtypes = [vp, i32, vp]
        L.zk_pool_device_free.restype = None
        L.zk_ctx_set_wire.argtypes = [vp, u32]
        L.zk_proof_pack.argtypes = [C.c_char_p, u64, vp, u64, C.POINTER(u64)]
        L.zk_proof_unpack.argtypes = [C.c_char_p, u64, vp, u64, C.POINTER(u64)]
        L.zk_ctx_copy_probe.argtypes = [vp, u32, C.c_size_t, i32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.zk_pool_host_alloc.argtypes = [vp, C.c_size_t]
        L.zk_pool_host_alloc.restype = vp
        L.zk_pool_host_free.argtypes = [vp]
        L.zk_pool_host_free.restype = None
        L.zk_pool_numa_node.argtypes = [vp, i32]
        L.zk_pool_shard_ms.argtypes = [vp, C.POINTER(C.c_float), i32]
        L.zk_pool_test_locality.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), i32]
        L.zk_test_field_op.argtypes = [vp, i32, i32, u64, C.c_char_p, C.c_char_p, vp]
        L.zk_test_tom_commit.argtypes = [vp, u64, C.c_char_p, C.c_char_p, vp]
        L.zk_test_tom_commit_shape.argtypes = [vp, u32, u64, C.c_char_p, C.c_char_p, vp]
        L.zk_test_p256_fixed_mul.argtypes = [vp, i32, u64, C.c_char_p, vp]
        L.zk_test_exp_sum.argtypes = [vp, C.c_uint32, i32, u64, C.c_char_p, vp, vp]
        L.zk_test_msm_sum.argtypes = [vp, u32, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.zk_test_pmsm_sum.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp]
        L.zk_test_sha256.argtypes = [vp, u64, u64, C.c_char_p, vp]
        L.zk_test_rng_draws.argtypes = [vp, u64, C.POINTER(ZkRng), u32, u32, vp]
        _lib = L
    return _lib


class PinnedBuffer:
    """Page-locked host memory from zk_host_alloc (include/zkattest.h): .ptr for the C ABI, .view as a ctypes byte array.
    With `pool`: zk_pool_host_alloc -- the per-shard regions are placed on the NUMA nodes of the shards' devices."""

    def __init__(self, nbytes, pool=None):
        self.nbytes = nbytes
        self._pooled = pool is not None
        self.ptr = lib().zk_pool_host_alloc(pool.h, nbytes) if self._pooled else lib().zk_host_alloc(nbytes)
        if not self.ptr:
            raise MemoryError('zk_%shost_alloc(%d) failed' % ('pool_' if self._pooled else '', nbytes))
        self.view = (C.c_uint8 * nbytes).from_address(self.ptr)

    def free(self):
        if self.ptr:
            self.view = None
            (lib().zk_pool_host_free if self._pooled else lib().zk_host_free)(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ZkError(RuntimeError):
    def __init__(self, status, detail=''):
        self.status = status
        super().__init__('%s (status %d)%s' % (STATUS_TEXT.get(status, '?'), status, (': ' + detail) if detail else ''))


MODE_REFERENCE, MODE_HARDENED = 0, 1
RING_TABLE_E, RING_DIGIT_PLANES, RING_TABLE_E_DIGITS, RING_KEY_TABLES, RING_ACTIVE = 1, 2, 4, 8, 16   # zk_ring_info flags
# zk_screen_batch: the bits of flags[b] (0 = prove this witness) and the index of a key that is not in the ring
SCREEN_KEY_NOT_ON_CURVE, SCREEN_SIG_RANGE, SCREEN_SIG_INVALID, SCREEN_NOT_IN_RING, SCREEN_RING_NOT_RESIDENT = 1, 2, 4, 8, 16
WHICH_NONE = 0xFFFFFFFF
ESCROW_RING_ANY = 0xFFFFFFFF   # zk_rings_escrow_open_batch: search every resident ring, ascending ids
# zk_recover_batch: the bits of flags[b] (0 = the key was recovered and is in the ring at which_out[b]); shared values mean what they mean for the screen
RECOVER_SIG_RANGE, RECOVER_NOT_IN_RING, RECOVER_RING_NOT_RESIDENT, RECOVER_NO_POINT = 2, 8, 16, 32


def hardened_h(tag=b''):
    """Nothing-up-my-sleeve NistGroup.h (64 bytes) and ProofGroup.h (72 bytes) of the hardened mode (zk_hardened_h; host-only)."""
    a, b = C.create_string_buffer(64), C.create_string_buffer(72)
    rc = lib().zk_hardened_h(bytes(tag), len(tag), a, b)
    if rc:
        raise ZkError(rc)
    return a.raw, b.raw


def _wire_convert(fn, raw):
    raw = bytes(raw)
    n = C.c_uint64()
    rc = fn(raw, len(raw), None, 0, C.byref(n))
    if rc not in (0, 12):
        raise ZkError(rc, 'not a structurally complete proof of that layout')
    out = C.create_string_buffer(n.value)
    rc = fn(raw, len(raw), out, n.value, C.byref(n))
    if rc:
        raise ZkError(rc, 'not a structurally complete proof of that layout')
    return out.raw[:n.value]


def pack_proof(zka1):
    """ZKA1 -> ZKA1P (33-byte Tom coordinates): zk_proof_pack"""
    return _wire_convert(lib().zk_proof_pack, zka1)


def unpack_proof(zka1p):
    """ZKA1P -> ZKA1: zk_proof_unpack"""
    return _wire_convert(lib().zk_proof_unpack, zka1p)


def write_json(proof_bytes):
    """ZKA1 proof -> JSON text; the writeJson(SignatureProofList, proof) of src/serde.ts:34-36."""
    L = lib()
    raw = bytes(proof_bytes)
    n = C.c_uint64()
    cap = 5 * len(raw) + 4096          # the text is ~3.5x the binary proof: one call in the common case
    for _ in range(2):
        buf = C.create_string_buffer(cap)
        rc = L.zk_proof_to_json(raw, len(raw), buf, cap, C.byref(n))
        if rc != 12:
            break
        cap = n.value
    if rc:
        raise ZkError(rc)
    return buf.raw[:n.value].decode()


def read_json(text):
    """JSON text -> ZKA1 proof; the readJson(SignatureProofList, text) of src/serde.ts:21-32 (throws on bad input)."""
    L = lib()
    raw = text.encode() if isinstance(text, str) else bytes(text)
    n = C.c_uint64()
    cap = len(raw) // 2 + 64            # two hex digits per byte at least: the binary proof is shorter than half the text
    buf = C.create_string_buffer(cap)
    rc = L.zk_proof_from_json(raw, len(raw), buf, cap, C.byref(n))
    if rc == 12:
        buf = C.create_string_buffer(n.value)
        rc = L.zk_proof_from_json(raw, len(raw), buf, n.value, C.byref(n))
    if rc:
        raise ZkError(rc)
    return buf.raw[:n.value]


def _json_batch(fn, blob, off, n, cap, threads):
    L = lib()
    out_off, st = (C.c_uint64 * (n + 1))(), (C.c_int32 * n)()
    src = (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(blob or b'\0')
    for _ in range(2):
        out = (C.c_uint8 * max(cap, 1))()
        rc = fn(n, src, off, out, cap, out_off, st, threads)
        if rc != 12:
            break
        cap = out_off[n]
    if rc:
        raise ZkError(rc)
    return out, out_off, st


def write_json_batch(proofs, threads=0):
    """n ZKA1 proofs -> n JSON texts on `threads` host threads (0 = all): zk_proofs_to_json_batch.  -> (texts as bytes, statuses)."""
    n = len(proofs)
    off = (C.c_uint64 * (n + 1))()
    for i, p in enumerate(proofs):
        off[i + 1] = off[i] + len(p)
    out, toff, st = _json_batch(lib().zk_proofs_to_json_batch, b''.join(proofs), off, n, int(3.7 * off[n]) + 4096 * n, threads)
    raw = memoryview(out)
    return [bytes(raw[toff[i]:toff[i + 1]]) for i in range(n)], list(st)


def read_json_batch(texts, threads=0):
    """n JSON texts -> n ZKA1 proofs (b'' where a text does not parse: see the statuses): zk_proofs_from_json_batch."""
    texts = [t.encode() if isinstance(t, str) else bytes(t) for t in texts]
    n = len(texts)
    off = (C.c_uint64 * (n + 1))()
    for i, t in enumerate(texts):
        off[i + 1] = off[i] + len(t)
    out, poff, st = _json_batch(lib().zk_proofs_from_json_batch, b''.join(texts), off, n, off[n] // 3 + 64 * n, threads)
    raw = memoryview(out)
    return [bytes(raw[poff[i]:poff[i + 1]]) for i in range(n)], list(st)


class Engine:
    """One engine = one GPU (zk_ctx)."""

    def __init__(self, device=0, _borrowed=None):
        self.L = lib()
        self.sec = None
        self._keep = []
        self._owned = _borrowed is None
        if _borrowed is not None:   # a context owned by a Pool
            self.h = C.c_void_p(_borrowed)
            return
        h = C.c_void_p()
        rc = self.L.zk_ctx_create(device, C.byref(h))
        self.h = h
        self._chk(rc)

    def _chk(self, rc):
        if rc:
            detail = self.L.zk_last_error(self.h).decode()   # NULL handle: why zk_ctx_create failed (thread-local in the library)
            raise ZkError(rc, detail)

    def close(self):
        if getattr(self, 'h', None):
            if self._owned:
                self.L.zk_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, nist_h64, tom_g72, tom_h72, sec_level=80):
        self._chk(self.L.zk_ctx_set_params(self.h, bytes(nist_h64), bytes(tom_g72), bytes(tom_h72), sec_level))
        self.sec = sec_level

    def set_ring(self, keys_be32, nkeys=None):
        keys_be32 = bytes(keys_be32)
        if nkeys is None:
            nkeys = len(keys_be32) // 32
        self._chk(self.L.zk_ctx_set_ring(self.h, keys_be32, nkeys))

    def keys_to_ints(self, pk_xy64):
        """keyToInt for n keys (64-byte affine each): (n x 32-byte big-endian ring entries, list of statuses)."""
        pk_xy64 = bytes(pk_xy64)
        n = len(pk_xy64) // 64
        out = C.create_string_buffer(32 * n)
        st = (C.c_int32 * n)()
        self._chk(self.L.zk_keys_to_ints(self.h, n, pk_xy64, out, st))
        return out.raw, list(st)

    def set_ring_device(self, dev_ptr, nkeys):
        self._chk(self.L.zk_ctx_set_ring_device(self.h, dev_ptr, nkeys))

    def set_chunk(self, chunk):
        self._chk(self.L.zk_ctx_set_chunk(self.h, chunk))

    def set_lanes(self, lanes):
        self._chk(self.L.zk_ctx_set_lanes(self.h, lanes))

    def set_mode(self, mode):
        """MODE_REFERENCE (default, byte parity with the reference) or MODE_HARDENED (statement hashed into the GK challenge)."""
        self._chk(self.L.zk_ctx_set_mode(self.h, int(mode)))

    def set_verify_level(self, per_proof):
        """zk_ctx_set_verify_level: False / 0 = every proof at the context's secLevel (default), True / 1 = every proof at its own header's
        secLevel, as the reference's verifySignatureList does."""
        self._chk(self.L.zk_ctx_set_verify_level(self.h, 1 if per_proof else 0))

    def set_verify_reps(self, all):
        """zk_ctx_set_verify_reps: False / 0 = the 20 repetitions generateIndices samples (default, the reference's verifier), True / 1 = every
        repetition of every proof, in ceil(secLevel / 20) passes (stricter than the reference; blocking calls only)."""
        self._chk(self.L.zk_ctx_set_verify_reps(self.h, 1 if all else 0))

    def ring_digest(self):
        d = C.create_string_buffer(32)
        self._chk(self.L.zk_ring_digest(self.h, d))
        return d.raw

    def add_ring(self, keys_be32, nkeys=None):
        """zk_ctx_add_ring: builds a new resident ring (not made active) and returns its id."""
        keys_be32 = bytes(keys_be32)
        rid = C.c_uint32()
        self._chk(self.L.zk_ctx_add_ring(self.h, keys_be32, nkeys if nkeys is not None else len(keys_be32) // 32, C.byref(rid)))
        return rid.value

    def add_ring_device(self, dev_ptr, nkeys):
        rid = C.c_uint32()
        self._chk(self.L.zk_ctx_add_ring_device(self.h, dev_ptr, nkeys, C.byref(rid)))
        return rid.value

    def use_ring(self, ring):
        """zk_ctx_use_ring: makes a resident ring the active one (no rebuild)."""
        self._chk(self.L.zk_ctx_use_ring(self.h, ring))

    def drop_ring(self, ring):
        self._chk(self.L.zk_ctx_drop_ring(self.h, ring))

    def update_ring(self, ring, changes, nkeys=None):
        """zk_ctx_update_ring: the resident ring becomes what set_ring of the changed key list would build, rewriting only what the change touches.
        changes: dict {index: key} or list of (index, key) (a later entry for the same index wins); nkeys: the new key count (default: unchanged)."""
        cnt, idx, keys = _ring_changes(changes)
        if nkeys is None:
            nkeys = self.ring_info(ring)['n_keys']
        self._chk(self.L.zk_ctx_update_ring(self.h, ring, cnt, idx, keys, nkeys))

    def ring_info(self, ring):
        """zk_ring_info: dict with n_keys, log_n, flags (RING_* bits) and generation."""
        nk, ln, fl, gen = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._chk(self.L.zk_ring_info(self.h, ring, C.byref(nk), C.byref(ln), C.byref(fl), C.byref(gen)))
        return {'n_keys': nk.value, 'log_n': ln.value, 'flags': fl.value, 'generation': gen.value}

    def verify_batch_rings(self, msg, proofs, ring_ids, vseeds=None):
        """zk_verify_batch_rings: verify_batch with one resident ring id per proof."""
        B = len(proofs)
        off = (C.c_uint64 * (B + 1))()
        o = 0
        for b, p in enumerate(proofs):
            off[b] = o
            o += len(p)
        off[B] = o
        ids = (C.c_uint32 * max(B, 1))(*ring_ids)
        ok = (C.c_uint8 * B)()
        st = (C.c_int32 * B)()
        self._chk(self.L.zk_verify_batch_rings(self.h, B, bytes(msg), b''.join(proofs), off, ids, bytes(vseeds) if vseeds is not None else None, ok, st))
        return list(ok), list(st)

    def verify_batch_rings_device(self, B, d_msg, d_proofs, d_off, d_ring_ids, d_vseeds, d_ok, d_status):
        self._chk(self.L.zk_verify_batch_rings_device(self.h, B, d_msg, d_proofs, d_off, d_ring_ids, d_vseeds, d_ok, d_status))

    def set_verify_groups(self, groups):
        self._chk(self.L.zk_ctx_set_verify_groups(self.h, groups))

    def set_ring_fold(self, matrix_pipe):
        self._chk(self.L.zk_ctx_set_ring_fold(self.h, 1 if matrix_pipe else 0))

    def set_wire(self, packed):
        """zk_ctx_set_wire: False / 0 = ZKA1, True / 1 = ZKA1P (33-byte Tom coordinates) for what the prover emits and the verifier is handed"""
        self._chk(self.L.zk_ctx_set_wire(self.h, 1 if packed else 0))

    def set_slice(self, proofs):
        """Proofs per PointAdd slice of the prover (0 = automatic: 4096 with page-locked output, none otherwise)."""
        self._chk(self.L.zk_ctx_set_slice(self.h, int(proofs)))

    def set_host_taper(self, on):
        """Tapered chunk plan of the host-pointer calls on page-locked buffers (default on)."""
        self._chk(self.L.zk_ctx_set_host_taper(self.h, 1 if on else 0))

    def set_comb_bits(self, bits):
        """Comb width of the Tom-256 fixed-base tables (8..24 unsigned, 25/26 signed digits); call before set_params."""
        self._chk(self.L.zk_ctx_set_comb_bits(self.h, bits))

    def wipe(self):
        """zero the witness-derived device memory of the context (prover workspaces, staged inputs); also done by close() and after a failed prove call"""
        self.L.zk_ctx_wipe.argtypes = [C.c_void_p]
        self.L.zk_ctx_wipe.restype = C.c_int
        self._chk(self.L.zk_ctx_wipe(self.h))

    def set_batch_verify(self, min_chunk):
        """Chunks of >= min_chunk proofs (default 256; 0 never, 1 always) get the chunk-wide bucket-method check of the
        Tom-256 relations first; the per-proof sums only run when it fails."""
        self._chk(self.L.zk_ctx_set_batch_verify(self.h, int(min_chunk)))

    def proof_max_size(self):
        return self.L.zk_proof_max_size(self.h)

    def prove_batch(self, msg, sig, pk, which, seeds=None, streams=None, stream_blocks=0):
        """Host-buffer entry point.  Returns (list of proof bytes or None, list of status).
        seeds: B x 32 bytes, FRESH, SECRET and distinct per proof (every blinding factor of proof b derives from seed b: a
        reused or guessable seed reveals the witness).  With neither seeds nor streams the seeds come from os.urandom."""
        B = len(which)
        if seeds is None and streams is None:
            seeds = os.urandom(32 * B)
        if streams is None and len(seeds) != 32 * B:
            raise ValueError('seeds must hold 32 bytes per proof')
        cap = self.proof_max_size() * max(B, 1)
        out = C.create_string_buffer(cap)
        off = (C.c_uint64 * (B + 1))()
        st = (C.c_int32 * B)()
        w = (C.c_uint32 * B)(*which)
        if streams is None:
            data = C.create_string_buffer(bytes(seeds), 32 * B)
            rng = ZkRng(0, C.cast(data, C.c_void_p), 0)
        else:
            data = C.create_string_buffer(bytes(streams), 32 * B * stream_blocks)
            rng = ZkRng(1, C.cast(data, C.c_void_p), stream_blocks)
        self._chk(self.L.zk_prove_batch(self.h, B, bytes(msg), bytes(sig), bytes(pk), w, C.byref(rng), out, cap, off, st))
        raw = out.raw
        proofs = [raw[off[b]:off[b + 1]] if st[b] == 0 else None for b in range(B)]
        return proofs, list(st)

    def ring_proof_max_size(self, ring):
        """zk_ring_proof_max_size: upper bound of one proof's size over a resident ring (0 for an id that is not resident)"""
        return int(self.L.zk_ring_proof_max_size(self.h, ring))

    def _rings_cap(self, B, ring_ids):
        """bytes that hold B proofs over the resident rings among ring_ids (ids that are not resident give empty proofs)"""
        return max([self.ring_proof_max_size(r) for r in set(ring_ids)] + [32]) * max(B, 1)

    def prove_batch_rings(self, msg, sig, pk, which, ring_ids, seeds=None, streams=None, stream_blocks=0, cap=None, out=None):
        """zk_prove_batch_rings: prove_batch with one resident ring id per proof (which[b] indexes ring ring_ids[b]); the active ring plays no part.
        Returns (list of proof bytes or None, list of status); the proofs lie back to back in index order.  cap: the out_cap handed to the call
        (default: room for every proof); out: a PinnedBuffer to prove into (default: a pageable buffer)."""
        B = len(which)
        if len(ring_ids) != B:
            raise ValueError('one ring id per proof')
        if seeds is None and streams is None:
            seeds = os.urandom(32 * B)
        if streams is None and len(seeds) != 32 * B:
            raise ValueError('seeds must hold 32 bytes per proof')
        if cap is None:
            cap = self._rings_cap(B, ring_ids)
        if out is None:
            buf = C.create_string_buffer(max(cap, 1))
            optr = C.cast(buf, C.c_void_p)
        else:
            cap, optr = min(cap, out.nbytes), out.ptr
        off = (C.c_uint64 * (B + 1))()
        st = (C.c_int32 * B)()
        w = (C.c_uint32 * max(B, 1))(*which)
        ids = (C.c_uint32 * max(B, 1))(*ring_ids)
        if streams is None:
            data = C.create_string_buffer(bytes(seeds), 32 * B)
            rng = ZkRng(0, C.cast(data, C.c_void_p), 0)
        else:
            data = C.create_string_buffer(bytes(streams), 32 * B * stream_blocks)
            rng = ZkRng(1, C.cast(data, C.c_void_p), stream_blocks)
        self._chk(self.L.zk_prove_batch_rings(self.h, B, bytes(msg), bytes(sig), bytes(pk), w, ids, C.byref(rng), optr, cap, off, st))
        assert off[0] == 0 and all(off[b] <= off[b + 1] for b in range(B))
        raw = C.string_at(optr, off[B])
        return [raw[off[b]:off[b + 1]] if st[b] == 0 else None for b in range(B)], list(st)

    def prove_batch_rings_device(self, B, d_msg, d_sig, d_pk, d_which, d_ring_ids, d_seeds, d_out, out_cap, d_off, d_status, mode=0, stride_blocks=0):
        """zk_prove_batch_rings_device: every pointer a device address"""
        rng = ZkRng(mode, d_seeds, stride_blocks)
        self._chk(self.L.zk_prove_batch_rings_device(self.h, B, d_msg, d_sig, d_pk, d_which, d_ring_ids, C.byref(rng), d_out, out_cap, d_off, d_status))

    def screen_batch(self, msg, sig, pk, which=None, ring_ids=None):
        """zk_screen_batch / zk_screen_batch_rings: is each witness worth a proof?  Returns (which_out list, flags list): flags[b] is a set of SCREEN_*
        bits, 0 = the signature verifies and the key is in the ring at which_out[b].  which=None finds the lowest index of pk.x among the ring's keys
        (WHICH_NONE and SCREEN_NOT_IN_RING when absent), a list is checked entry by entry.  ring_ids: one resident ring id per witness instead of the
        active ring.  SCREEN_SIG_RANGE is stricter than the prover, which reduces r and s mod n."""
        B = len(bytes(msg)) // 32
        if len(sig) != 64 * B or len(pk) != 64 * B or (which is not None and len(which) != B) or (ring_ids is not None and len(ring_ids) != B):
            raise ValueError('32 bytes of hash, 64 of signature and 64 of key per witness, one index and one ring id each where given')
        w = (C.c_uint32 * max(B, 1))(*which) if which is not None else None
        wo = (C.c_uint32 * max(B, 1))()
        fl = (C.c_uint32 * max(B, 1))()
        if ring_ids is None:
            self._chk(self.L.zk_screen_batch(self.h, B, bytes(msg), bytes(sig), bytes(pk), w, wo, fl))
        else:
            ids = (C.c_uint32 * max(B, 1))(*ring_ids)
            self._chk(self.L.zk_screen_batch_rings(self.h, B, bytes(msg), bytes(sig), bytes(pk), w, ids, wo, fl))
        return list(wo)[:B], list(fl)[:B]

    def screen_batch_device(self, B, d_msg, d_sig, d_pk, d_which, d_which_out, d_flags, d_ring_ids=None):
        """zk_screen_batch_device / zk_screen_batch_rings_device: every pointer a device address (d_which may be None: find mode); d_which_out is what
        prove_batch_device takes as d_which"""
        if d_ring_ids is None:
            self._chk(self.L.zk_screen_batch_device(self.h, B, d_msg, d_sig, d_pk, d_which, d_which_out, d_flags))
        else:
            self._chk(self.L.zk_screen_batch_rings_device(self.h, B, d_msg, d_sig, d_pk, d_which, d_ring_ids, d_which_out, d_flags))

    def recover_batch(self, msg, sig, ring_ids=None):
        """zk_recover_batch / zk_recover_batch_rings: the signer's key from (msgHash, signature) alone and its index in the ring.  Returns (pk list, which_out
        list, flags list): flags[b] is a set of RECOVER_* bits; 0 = pk[b] (64 bytes x || y) is the key at which_out[b] and the witness (msg, sig, pk[b],
        which_out[b]) is what prove_batch takes; otherwise pk[b] is None and which_out[b] is WHICH_NONE.  ring_ids: one resident ring id per witness instead
        of the active ring."""
        B = len(bytes(msg)) // 32
        if len(msg) != 32 * B or len(sig) != 64 * B or (ring_ids is not None and len(ring_ids) != B):
            raise ValueError('32 bytes of hash and 64 of signature per witness, one ring id each where given')
        pk = (C.c_uint8 * max(64 * B, 1))()
        wo = (C.c_uint32 * max(B, 1))()
        fl = (C.c_uint32 * max(B, 1))()
        if ring_ids is None:
            self._chk(self.L.zk_recover_batch(self.h, B, bytes(msg), bytes(sig), pk, wo, fl))
        else:
            ids = (C.c_uint32 * max(B, 1))(*ring_ids)
            self._chk(self.L.zk_recover_batch_rings(self.h, B, bytes(msg), bytes(sig), ids, pk, wo, fl))
        raw = bytes(pk)
        return [raw[64 * b:64 * b + 64] if fl[b] == 0 else None for b in range(B)], list(wo)[:B], list(fl)[:B]

    def recover_batch_device(self, B, d_msg, d_sig, d_pk_out, d_which_out, d_flags, d_ring_ids=None):
        """zk_recover_batch_device / zk_recover_batch_rings_device: every pointer a device address; d_pk_out (64 B bytes) and d_which_out are what
        prove_batch_device takes as d_pk and d_which"""
        if d_ring_ids is None:
            self._chk(self.L.zk_recover_batch_device(self.h, B, d_msg, d_sig, d_pk_out, d_which_out, d_flags))
        else:
            self._chk(self.L.zk_recover_batch_rings_device(self.h, B, d_msg, d_sig, d_ring_ids, d_pk_out, d_which_out, d_flags))

    def test_set_prove_segment(self, proofs):
        """test build only (lib/libzkattest_hip_testhooks.so through ZKATTEST_LIB): proofs per segment of the mixed-ring prove calls; 0 = the default"""
        if not hasattr(self.L, 'zk_test_set_prove_segment'):
            raise RuntimeError('this build has no test hooks (load lib/libzkattest_hip_testhooks.so through ZKATTEST_LIB)')
        self.L.zk_test_set_prove_segment.argtypes = [C.c_void_p, C.c_uint32]
        self._chk(self.L.zk_test_set_prove_segment(self.h, int(proofs)))

    def prove_batch_host_raw(self, msg, sig, pk, which, seeds, out=None):
        """zk_prove_batch on host buffers without slicing the output.  out: a PinnedBuffer (overlapped DMA), a ctypes byte array
        (pageable) or None (a pageable array is allocated).  Returns (wall seconds of the C call, out buffer, offsets, statuses)."""
        import time
        B = len(which)
        cap = self.proof_max_size() * max(B, 1)
        if out is None:
            out = (C.c_uint8 * cap)()
        if isinstance(out, PinnedBuffer):
            cap, optr = min(cap, out.nbytes), out.ptr
        else:
            cap, optr = min(cap, C.sizeof(out)), C.addressof(out)
        off = (C.c_uint64 * (B + 1))()
        st = (C.c_int32 * B)()
        w = (C.c_uint32 * B)(*which)
        data = C.create_string_buffer(bytes(seeds), 32 * B)
        rng = ZkRng(0, C.cast(data, C.c_void_p), 0)
        msg, sig, pk = bytes(msg), bytes(sig), bytes(pk)
        t0 = time.time()
        self._chk(self.L.zk_prove_batch(self.h, B, msg, sig, pk, w, C.byref(rng), optr, cap, off, st))
        return time.time() - t0, out, off, st

    def verify_batch_host_raw(self, msg, proofs, off, B, vseeds=None):
        """zk_verify_batch on a packed host buffer (PinnedBuffer or ctypes array) with offsets `off`.  Returns (seconds, ok, status)."""
        import time
        ok = (C.c_uint8 * B)()
        st = (C.c_int32 * B)()
        ptr = proofs.ptr if isinstance(proofs, PinnedBuffer) else C.addressof(proofs)
        msg = bytes(msg)
        t0 = time.time()
        self._chk(self.L.zk_verify_batch(self.h, B, msg, ptr, off, bytes(vseeds) if vseeds is not None else None, ok, st))
        return time.time() - t0, ok, st

    # ---- streamed calls (zk_prove_submit / zk_prove_wait ...): several batches in flight, waits in submission order
    def prove_submit(self, msg, sig, pk, which, seeds, out):
        """Queues one batch; `out` is a PinnedBuffer.  Returns a ticket for prove_wait (it keeps every buffer of the job alive)."""
        B = len(which)
        t = {'B': B, 'out': out, 'off': (C.c_uint64 * (B + 1))(), 'st': (C.c_int32 * B)(), 'w': (C.c_uint32 * B)(*which),
             'data': C.create_string_buffer(bytes(seeds), 32 * B), 'msg': bytes(msg), 'sig': bytes(sig), 'pk': bytes(pk), 'job': C.c_void_p()}
        t['rng'] = ZkRng(0, C.cast(t['data'], C.c_void_p), 0)
        cap = min(self.proof_max_size() * max(B, 1), out.nbytes)
        self._chk(self.L.zk_prove_submit(self.h, B, t['msg'], t['sig'], t['pk'], t['w'], C.byref(t['rng']), out.ptr, cap, t['off'], t['st'], C.byref(t['job'])))
        return t

    def prove_wait(self, t):
        """-> (offsets, statuses) of the ticket's batch; the proofs are in the ticket's PinnedBuffer."""
        self._chk(self.L.zk_prove_wait(self.h, t['job']))
        return t['off'], t['st']

    def verify_submit(self, msg, proofs, off, B, vseeds=None):
        t = {'B': B, 'proofs': proofs, 'off': off, 'ok': (C.c_uint8 * B)(), 'st': (C.c_int32 * B)(), 'msg': bytes(msg),
             'seeds': bytes(vseeds) if vseeds is not None else None, 'job': C.c_void_p()}
        self._chk(self.L.zk_verify_submit(self.h, B, t['msg'], proofs.ptr, off, t['seeds'], t['ok'], t['st'], C.byref(t['job'])))
        return t

    def verify_wait(self, t):
        self._chk(self.L.zk_verify_wait(self.h, t['job']))
        return t['ok'], t['st']

    def copy_probe(self, lane=0, nbytes=256 << 20, numa_node=-1):
        """(d2h GB/s, h2d GB/s) of a page-locked copy on that lane's copy stream (zk_ctx_copy_probe); numa_node >= 0 binds the host buffer"""
        a, b = C.c_float(), C.c_float()
        self._chk(self.L.zk_ctx_copy_probe(self.h, lane, nbytes, numa_node, C.byref(a), C.byref(b)))
        return round(a.value, 1), round(b.value, 1)

    def test_counter(self, which=0):
        return int(self.L.zk_test_counter(self.h, which))

    def set_key_tables(self, on):
        self._chk(self.L.zk_ctx_set_key_tables(self.h, 1 if on else 0))

    def prove_submit_device(self, B, d_msg, d_sig, d_pk, d_which, d_seeds, d_out, out_cap, d_off, d_status, mode=0, stride_blocks=0):
        """zk_prove_submit_device: every pointer a device address; returns the ticket for prove_wait."""
        t = {'rng': ZkRng(mode, d_seeds, stride_blocks), 'job': C.c_void_p(), 'off': None, 'st': None}
        self._chk(self.L.zk_prove_submit_device(self.h, B, d_msg, d_sig, d_pk, d_which, C.byref(t['rng']), d_out, out_cap, d_off, d_status, C.byref(t['job'])))
        return t

    def prove_batch_device(self, B, d_msg, d_sig, d_pk, d_which, d_seeds, d_out, out_cap, d_off, d_status, mode=0, stride_blocks=0):
        rng = ZkRng(mode, d_seeds, stride_blocks)
        self._chk(self.L.zk_prove_batch_device(self.h, B, d_msg, d_sig, d_pk, d_which, C.byref(rng), d_out, out_cap, d_off, d_status))

    def verify_batch(self, msg, proofs, vseeds=None):
        B = len(proofs)
        off = (C.c_uint64 * (B + 1))()
        o = 0
        for b, p in enumerate(proofs):
            off[b] = o
            o += len(p)
        off[B] = o
        ok = (C.c_uint8 * B)()
        st = (C.c_int32 * B)()
        self._chk(self.L.zk_verify_batch(self.h, B, bytes(msg), b''.join(proofs), off, bytes(vseeds) if vseeds is not None else None, ok, st))
        return list(ok), list(st)

    def verify_batch_device(self, B, d_msg, d_proofs, d_off, d_vseeds, d_ok, d_status):
        self._chk(self.L.zk_verify_batch_device(self.h, B, d_msg, d_proofs, d_off, d_vseeds, d_ok, d_status))

    # ---- ring membership of a committed value on its own (zk_member_*): proveMembership / verifyMembership on the active ring, "ZKM1" proofs
    def member_proof_size(self, ring=None):
        """bytes of one ZKM1 proof over the active ring (ring=None; 0 without one) or over the resident ring `ring` (0 for an id that is not resident):
        16 + 288 n + 32 (3 n + 1)"""
        if ring is not None:
            return int(self.L.zk_member_proof_size_ring(self.h, int(ring)))
        return int(self.L.zk_member_proof_size(self.h))

    @staticmethod
    def _member_context(context, B):
        """context of a bound membership call: B x 32 bytes, or a list of B 32-byte strings -> bytes (never empty: NULL means 'no context' to the C ABI)"""
        if not isinstance(context, (bytes, bytearray, memoryview)):
            context = b''.join(bytes(x) for x in context)
        if len(context) != 32 * B:
            raise ValueError('context must hold 32 bytes per proof')
        return bytes(context) if B else bytes(32)

    def member_prove_batch(self, which, blinders=None, seeds=None, streams=None, stream_blocks=0, want_blinders=True, context=None):
        """One membership proof per entry of `which` (indices into the padded active ring).  context (B x 32 bytes, or a list of 32-byte strings): bound
        proofs, "ZKMB" -- the challenge also hashes the ring's digest, context[b] and com[b] (zk_member_prove_batch_bound); None: "ZKM1".  blinders: B x 32 bytes, the openings' blinders (reduced mod
        q), or None: the engine draws each from fill 0 of the proof's RNG.  Returns (proofs: list of bytes or None, coms: list of 72-byte Tom-256 points,
        blinders: list of 32-byte scalars or None, statuses).  seeds: as in prove_batch -- fresh, secret, one per proof."""
        B = len(which)
        if seeds is None and streams is None:
            seeds = os.urandom(32 * B)
        if streams is None and len(seeds) != 32 * B:
            raise ValueError('seeds must hold 32 bytes per proof')
        if blinders is not None and len(blinders) != 32 * B:
            raise ValueError('blinders must hold 32 bytes per proof')
        size = self.member_proof_size()
        out = C.create_string_buffer(max(size * B, 1))
        com = C.create_string_buffer(max(72 * B, 1))
        bo = C.create_string_buffer(max(32 * B, 1)) if want_blinders else None
        st = (C.c_int32 * max(B, 1))()
        w = (C.c_uint32 * max(B, 1))(*which)
        if streams is None:
            data = C.create_string_buffer(bytes(seeds), max(32 * B, 1))
            rng = ZkRng(0, C.cast(data, C.c_void_p), 0)
        else:
            data = C.create_string_buffer(bytes(streams), max(32 * B * stream_blocks, 1))
            rng = ZkRng(1, C.cast(data, C.c_void_p), stream_blocks)
        bl = bytes(blinders) if blinders is not None else None
        if context is None:
            self._chk(self.L.zk_member_prove_batch(self.h, B, w, bl, C.byref(rng), com, bo, out, size * B, st))
        else:
            self._chk(self.L.zk_member_prove_batch_bound(self.h, B, w, self._member_context(context, B), bl, C.byref(rng), com, bo, out, size * B, st))
        raw, craw = out.raw, com.raw
        proofs = [raw[size * b:size * (b + 1)] if st[b] == 0 else None for b in range(B)]
        self.member_last_raw = raw[:size * B]   # the B slots as written (a slot whose status is not 0 is zero-filled)
        return (proofs, [craw[72 * b:72 * (b + 1)] for b in range(B)], [bo.raw[32 * b:32 * (b + 1)] for b in range(B)] if want_blinders else None,
                list(st)[:B])

    def member_prove_batch_device(self, B, d_which, d_blinders, d_rng, d_com, d_blinders_out, d_out, out_cap, d_status, mode=0, stride_blocks=0, d_context=None):
        rng = ZkRng(mode, d_rng, stride_blocks)
        if d_context is None:
            self._chk(self.L.zk_member_prove_batch_device(self.h, B, d_which, d_blinders, C.byref(rng), d_com, d_blinders_out, d_out, out_cap, d_status))
        else:
            self._chk(self.L.zk_member_prove_batch_bound_device(self.h, B, d_which, d_context, d_blinders, C.byref(rng), d_com, d_blinders_out, d_out, out_cap, d_status))

    def member_verify_batch(self, coms, proofs, vseeds=None, context=None):
        """verifyMembership for B (com, proof) pairs on the active ring; every proof is member_proof_size() bytes.  context: as in member_prove_batch --
        the bound verifier (zk_member_verify_batch_bound), which takes "ZKMB" proofs only.  Returns (ok list, status list)."""
        B = len(proofs)
        size = self.member_proof_size()
        if len(coms) != B or any(len(p) != size for p in proofs) or any(len(cm) != 72 for cm in coms):
            raise ValueError('one 72-byte commitment and one proof of member_proof_size() bytes per entry')
        ok = (C.c_uint8 * max(B, 1))()
        st = (C.c_int32 * max(B, 1))()
        vs = bytes(vseeds) if vseeds is not None else None
        if context is None:
            self._chk(self.L.zk_member_verify_batch(self.h, B, b''.join(coms), b''.join(proofs), vs, ok, st))
        else:
            self._chk(self.L.zk_member_verify_batch_bound(self.h, B, b''.join(coms), self._member_context(context, B), b''.join(proofs), vs, ok, st))
        return list(ok)[:B], list(st)[:B]

    def member_verify_batch_device(self, B, d_com, d_proofs, d_vseeds, d_ok, d_status, d_context=None):
        if d_context is None:
            self._chk(self.L.zk_member_verify_batch_device(self.h, B, d_com, d_proofs, d_vseeds, d_ok, d_status))
        else:
            self._chk(self.L.zk_member_verify_batch_bound_device(self.h, B, d_com, d_context, d_proofs, d_vseeds, d_ok, d_status))

    # ---- ... with one resident ring id per proof (zk_member_*_batch_rings): the active ring plays no part
    def member_prove_batch_rings(self, which, ring_ids, blinders=None, seeds=None, streams=None, stream_blocks=0, want_blinders=True, cap=None, context=None):
        """member_prove_batch with one resident ring id per proof (which[b] indexes ring ring_ids[b]; context: bound proofs, each over ITS ring's digest).  Returns (proofs: list of bytes or None, coms,
        blinders or None, statuses); the proofs lie back to back in index order: member_last_off holds the B + 1 offsets, member_last_raw the bytes.
        An id that is not resident gives status 14, no proof and 72 zero bytes of com.  cap: the out_cap handed to the call (default: what the batch takes)."""
        B = len(which)
        if len(ring_ids) != B:
            raise ValueError('one ring id per proof')
        if seeds is None and streams is None:
            seeds = os.urandom(32 * B)
        if streams is None and len(seeds) != 32 * B:
            raise ValueError('seeds must hold 32 bytes per proof')
        if blinders is not None and len(blinders) != 32 * B:
            raise ValueError('blinders must hold 32 bytes per proof')
        if cap is None:
            sizes = {r: self.member_proof_size(r) for r in set(ring_ids)}
            cap = sum(sizes[r] for r in ring_ids)
        out = C.create_string_buffer(max(cap, 1))
        com = C.create_string_buffer(max(72 * B, 1))
        bo = C.create_string_buffer(max(32 * B, 1)) if want_blinders else None
        st = (C.c_int32 * max(B, 1))()
        off = (C.c_uint64 * (B + 1))()
        w = (C.c_uint32 * max(B, 1))(*which)
        ids = (C.c_uint32 * max(B, 1))(*ring_ids)
        if streams is None:
            data = C.create_string_buffer(bytes(seeds), max(32 * B, 1))
            rng = ZkRng(0, C.cast(data, C.c_void_p), 0)
        else:
            data = C.create_string_buffer(bytes(streams), max(32 * B * stream_blocks, 1))
            rng = ZkRng(1, C.cast(data, C.c_void_p), stream_blocks)
        bl = bytes(blinders) if blinders is not None else None
        if context is None:
            self._chk(self.L.zk_member_prove_batch_rings(self.h, B, w, ids, bl, C.byref(rng), com, bo, out, cap, off, st))
        else:
            self._chk(self.L.zk_member_prove_batch_rings_bound(self.h, B, w, self._member_context(context, B), ids, bl, C.byref(rng), com, bo, out, cap, off, st))
        raw, craw = out.raw, com.raw
        self.member_last_off = list(off)
        self.member_last_raw = raw[:off[B]]
        proofs = [raw[off[b]:off[b + 1]] if st[b] == 0 else None for b in range(B)]
        return (proofs, [craw[72 * b:72 * (b + 1)] for b in range(B)], [bo.raw[32 * b:32 * (b + 1)] for b in range(B)] if want_blinders else None,
                list(st)[:B])

    def member_prove_batch_rings_device(self, B, d_which, d_ring_ids, d_blinders, d_rng, d_com, d_blinders_out, d_out, out_cap, d_off, d_status, mode=0, stride_blocks=0,
                                        d_context=None):
        """zk_member_prove_batch_rings_device (d_context: zk_member_prove_batch_rings_bound_device): every pointer a device address"""
        rng = ZkRng(mode, d_rng, stride_blocks)
        if d_context is None:
            self._chk(self.L.zk_member_prove_batch_rings_device(self.h, B, d_which, d_ring_ids, d_blinders, C.byref(rng), d_com, d_blinders_out, d_out, out_cap, d_off, d_status))
        else:
            self._chk(self.L.zk_member_prove_batch_rings_bound_device(self.h, B, d_which, d_context, d_ring_ids, d_blinders, C.byref(rng), d_com, d_blinders_out, d_out, out_cap,
                                                                      d_off, d_status))

    def member_verify_batch_rings(self, coms, proofs, ring_ids, vseeds=None, offsets=None, context=None):
        """verifyMembership for B (com, proof) pairs, proof b under the resident ring ring_ids[b].  proofs: a list of byte strings laid back to back, or
        (offsets given) the bytes of the whole batch with its B + 1 offsets.  context: as in member_prove_batch -- the bound verifier
        (zk_member_verify_batch_rings_bound): "ZKMB" proofs only, proof b against the digest of ring ring_ids[b] and context[b].  Returns (ok list, status list)."""
        B = len(coms)
        if len(ring_ids) != B or any(len(cm) != 72 for cm in coms):
            raise ValueError('one 72-byte commitment and one ring id per entry')
        if offsets is None:
            if len(proofs) != B:
                raise ValueError('one proof per entry')
            offsets, run = [0], 0
            for p in proofs:
                run += len(p)
                offsets.append(run)
            proofs = b''.join(proofs)
        elif len(offsets) != B + 1:
            raise ValueError('B + 1 offsets')
        ok = (C.c_uint8 * max(B, 1))()
        st = (C.c_int32 * max(B, 1))()
        off = (C.c_uint64 * (B + 1))(*offsets)
        ids = (C.c_uint32 * max(B, 1))(*ring_ids)
        vs = bytes(vseeds) if vseeds is not None else None
        if context is None:
            self._chk(self.L.zk_member_verify_batch_rings(self.h, B, b''.join(coms), bytes(proofs), off, ids, vs, ok, st))
        else:
            self._chk(self.L.zk_member_verify_batch_rings_bound(self.h, B, b''.join(coms), self._member_context(context, B), bytes(proofs), off, ids, vs, ok, st))
        return list(ok)[:B], list(st)[:B]

    def member_verify_batch_rings_device(self, B, d_com, d_proofs, d_off, d_ring_ids, d_vseeds, d_ok, d_status, d_context=None):
        """zk_member_verify_batch_rings_device (d_context: zk_member_verify_batch_rings_bound_device): every pointer a device address"""
        if d_context is None:
            self._chk(self.L.zk_member_verify_batch_rings_device(self.h, B, d_com, d_proofs, d_off, d_ring_ids, d_vseeds, d_ok, d_status))
        else:
            self._chk(self.L.zk_member_verify_batch_rings_bound_device(self.h, B, d_com, d_context, d_proofs, d_off, d_ring_ids, d_vseeds, d_ok, d_status))

    # ---- re-ring (zk_prove_key_blinders, zk_proof_rering_batch): a ZKA1 proof moved to the active ring, its signature part untouched
    @staticmethod
    def _rng(B, seeds, streams, stream_blocks):
        if streams is None:
            if len(seeds) != 32 * B:
                raise ValueError('seeds must hold 32 bytes per proof')
            data = C.create_string_buffer(bytes(seeds), max(32 * B, 1))
            return ZkRng(0, C.cast(data, C.c_void_p), 0), data
        data = C.create_string_buffer(bytes(streams), max(32 * B * stream_blocks, 1))
        return ZkRng(1, C.cast(data, C.c_void_p), stream_blocks), data

    def prove_key_blinders(self, seeds=None, streams=None, stream_blocks=0):
        """zk_prove_key_blinders: the blinder of keyXcom in the proof prove_batch makes from the same seeds / streams (draw 1 of each proof), a list of
        32-byte scalars -- what rering_batch needs later.  As secret as the seeds."""
        B = (len(seeds) // 32) if streams is None else len(streams) // (32 * stream_blocks)
        rng, _keep = self._rng(B, seeds, streams, stream_blocks)
        out = C.create_string_buffer(max(32 * B, 1))
        self._chk(self.L.zk_prove_key_blinders(self.h, B, C.byref(rng), out))
        return [out.raw[32 * b:32 * b + 32] for b in range(B)]

    def prove_key_blinders_device(self, B, d_rng, d_out, mode=0, stride_blocks=0):
        rng = ZkRng(mode, d_rng, stride_blocks)
        self._chk(self.L.zk_prove_key_blinders_device(self.h, B, C.byref(rng), d_out))

    def rering_batch(self, msg, proofs, which_new, key_blinders, seeds=None, streams=None, stream_blocks=0, in_place=False, cap=None):
        """zk_proof_rering_batch: every proof (bytes, in the context's wire layout) with its GKProof section replaced by one for the ACTIVE ring, where
        ring[which_new[b]] is the proof's key and key_blinders[b] (32 bytes each, or B x 32 bytes) keyXcom's blinder (prove_key_blinders).  seeds / streams
        must be FRESH: never the ones the proofs were made with.  Returns (proofs: list of bytes, None where the status is not 0; statuses); the offsets the
        call wrote are kept in self.rering_last_off.  in_place: out == proofs, one buffer: allowed when every
        proof's n is the ring's (ZkError 14 otherwise); a failed proof then keeps its bytes and is returned as they are.  cap: the out_cap handed to the call."""
        B = len(proofs)
        if len(which_new) != B:
            raise ValueError('one index per proof')
        if not isinstance(key_blinders, (bytes, bytearray, memoryview)):
            key_blinders = b''.join(bytes(x) for x in key_blinders)
        if len(key_blinders) != 32 * B or len(msg) != 32 * B:
            raise ValueError('msg and key_blinders must hold 32 bytes per proof')
        if seeds is None and streams is None:
            seeds = os.urandom(32 * B)
        rng, data = self._rng(B, seeds, streams, stream_blocks)
        blob = b''.join(proofs)
        off = (C.c_uint64 * (B + 1))()
        o = 0
        for b, p in enumerate(proofs):
            off[b] = o
            o += len(p)
        off[B] = o
        w = (C.c_uint32 * max(B, 1))(*which_new)
        st = (C.c_int32 * max(B, 1))()
        out_off = (C.c_uint64 * (B + 1))()
        if in_place:   # one buffer for proofs and out: only the GKProof sections are rewritten, a failed proof keeps its bytes
            buf = C.create_string_buffer(blob, max(len(blob), 1))
            self._chk(self.L.zk_proof_rering_batch(self.h, B, bytes(msg), buf, off, w, bytes(key_blinders), C.byref(rng), buf, len(blob) if cap is None else cap, out_off, st))
            raw = buf.raw[:len(blob)]
            self.rering_last_off = list(out_off)
            return [raw[out_off[b]:out_off[b + 1]] for b in range(B)], list(st)[:B]
        if cap is None:
            cap = len(blob) + B * self.member_proof_size()   # every head as it is plus a new GKProof section (16 bytes to spare per proof)
        out = C.create_string_buffer(max(cap, 1))
        self._chk(self.L.zk_proof_rering_batch(self.h, B, bytes(msg), blob, off, w, bytes(key_blinders), C.byref(rng), out, cap, out_off, st))
        assert out_off[0] == 0 and all(out_off[b] <= out_off[b + 1] for b in range(B))
        raw = out.raw[:out_off[B]]
        self.rering_last_off = list(out_off)
        return [raw[out_off[b]:out_off[b + 1]] if st[b] == 0 else None for b in range(B)], list(st)[:B]

    def rering_batch_device(self, B, d_msg, d_proofs, d_off, d_which_new, d_key_blinders, d_rng, d_out, out_cap, d_out_off, d_status, mode=0, stride_blocks=0):
        """zk_proof_rering_batch_device: every pointer a device address; d_out == d_proofs re-rings in place"""
        rng = ZkRng(mode, d_rng, stride_blocks)
        self._chk(self.L.zk_proof_rering_batch_device(self.h, B, d_msg, d_proofs, d_off, d_which_new, d_key_blinders, C.byref(rng), d_out, out_cap, d_out_off, d_status))

    def rering_batch_rings(self, msg, proofs, which_new, ring_ids, key_blinders, seeds=None, streams=None, stream_blocks=0, in_place=False, cap=None):
        """zk_proof_rering_batch_rings: rering_batch with one resident ring id per proof -- proof b is moved to ring ring_ids[b], the active ring is neither
        read nor changed.  Every proof that passes the id, header and index checks has a slot of its own: a proof that then fails (opening, RNG stream) is
        returned as None and its slot holds zero bytes.  The offsets and the raw output are kept in self.rering_last_off / self.rering_last_raw.
        in_place: as in rering_batch, when every proof's n is its destination ring's."""
        B = len(proofs)
        if len(which_new) != B or len(ring_ids) != B:
            raise ValueError('one index and one ring id per proof')
        if not isinstance(key_blinders, (bytes, bytearray, memoryview)):
            key_blinders = b''.join(bytes(x) for x in key_blinders)
        if len(key_blinders) != 32 * B or len(msg) != 32 * B:
            raise ValueError('msg and key_blinders must hold 32 bytes per proof')
        if seeds is None and streams is None:
            seeds = os.urandom(32 * B)
        rng, data = self._rng(B, seeds, streams, stream_blocks)
        blob = b''.join(proofs)
        off = (C.c_uint64 * (B + 1))()
        o = 0
        for b, p in enumerate(proofs):
            off[b] = o
            o += len(p)
        off[B] = o
        w = (C.c_uint32 * max(B, 1))(*which_new)
        ids = (C.c_uint32 * max(B, 1))(*ring_ids)
        st = (C.c_int32 * max(B, 1))()
        out_off = (C.c_uint64 * (B + 1))()
        if in_place:
            buf = C.create_string_buffer(blob, max(len(blob), 1))
            self._chk(self.L.zk_proof_rering_batch_rings(self.h, B, bytes(msg), buf, off, w, ids, bytes(key_blinders), C.byref(rng), buf, len(blob) if cap is None else cap,
                                                         out_off, st))
            raw = buf.raw[:len(blob)]
            self.rering_last_off, self.rering_last_raw = list(out_off), raw
            return [raw[out_off[b]:out_off[b + 1]] for b in range(B)], list(st)[:B]
        if cap is None:   # every head as it is plus a GKProof section of the largest resident ring's size (n <= 63)
            cap = len(blob) + B * max([self.member_proof_size(r) for r in set(ring_ids)] + [0])
        out = C.create_string_buffer(max(cap, 1))
        self._chk(self.L.zk_proof_rering_batch_rings(self.h, B, bytes(msg), blob, off, w, ids, bytes(key_blinders), C.byref(rng), out, cap, out_off, st))
        assert out_off[0] == 0 and all(out_off[b] <= out_off[b + 1] for b in range(B))
        raw = out.raw[:out_off[B]]
        self.rering_last_off, self.rering_last_raw = list(out_off), raw
        return [raw[out_off[b]:out_off[b + 1]] if st[b] == 0 else None for b in range(B)], list(st)[:B]

    def rering_batch_rings_device(self, B, d_msg, d_proofs, d_off, d_which_new, d_ring_ids, d_key_blinders, d_rng, d_out, out_cap, d_out_off, d_status, mode=0, stride_blocks=0):
        """zk_proof_rering_batch_rings_device: every pointer a device address; d_out == d_proofs re-rings in place"""
        rng = ZkRng(mode, d_rng, stride_blocks)
        self._chk(self.L.zk_proof_rering_batch_rings_device(self.h, B, d_msg, d_proofs, d_off, d_which_new, d_ring_ids, d_key_blinders, C.byref(rng), d_out, out_cap,
                                                            d_out_off, d_status))

    # ---- link proofs (zk_link_*, zk_proof_key_commitments): two Tom-256 commitments hide the same key ("ZKL1", 256 bytes)
    def link_proof_size(self):
        return int(self.L.zk_link_proof_size())

    @staticmethod
    def _rows(x, width, B, what):
        if not isinstance(x, (bytes, bytearray, memoryview)):
            x = b''.join(bytes(v) for v in x)
        if len(x) != width * B:
            raise ValueError('%s must hold %d bytes per proof' % (what, width))
        return bytes(x) if B else bytes(width)

    def link_prove_batch(self, keys, com1, blinder1, com2, blinder2, seeds=None, streams=None, stream_blocks=0, cap=None):
        """zk_link_prove_batch: proof b shows that com1[b] = keys[b] g + blinder1[b] h and com2[b] = keys[b] g + blinder2[b] h hide one key.  keys, blinders:
        32-byte big-endian scalars (a list, or B x 32 bytes), coms: 72-byte Tom-256 points.  seeds / streams must be FRESH: never the ones either commitment's
        proof was made with.  Returns (proofs: list of 256-byte strings, None where the status is not 0; statuses).  Two debugging aids, as
        rering_batch and member_prove_batch have them: self.link_last_raw keeps the B slots as the call wrote them (a slot whose status is not 0 is zero-filled),
        and cap overrides the out_cap handed to the call (default 256 B; a smaller one makes the call refuse with ZK_E_BUFFER)."""
        B = len(keys) // 32 if isinstance(keys, (bytes, bytearray, memoryview)) else len(keys)
        k, c1, b1, c2, b2 = (self._rows(keys, 32, B, 'keys'), self._rows(com1, 72, B, 'com1'), self._rows(blinder1, 32, B, 'blinder1'),
                             self._rows(com2, 72, B, 'com2'), self._rows(blinder2, 32, B, 'blinder2'))
        if seeds is None and streams is None:
            seeds = os.urandom(32 * B)
        rng, _keep = self._rng(B, seeds, streams, stream_blocks)
        size = self.link_proof_size()
        out = C.create_string_buffer(max(size * B, 1))
        st = (C.c_int32 * max(B, 1))()
        self._chk(self.L.zk_link_prove_batch(self.h, B, k, c1, b1, c2, b2, C.byref(rng), out, size * B if cap is None else cap, st))
        raw = out.raw
        self.link_last_raw = raw[:size * B]
        return [raw[size * b:size * (b + 1)] if st[b] == 0 else None for b in range(B)], list(st)[:B]

    def link_prove_batch_device(self, B, d_keys, d_com1, d_blinder1, d_com2, d_blinder2, d_rng, d_out, out_cap, d_status, mode=0, stride_blocks=0):
        rng = ZkRng(mode, d_rng, stride_blocks)
        self._chk(self.L.zk_link_prove_batch_device(self.h, B, d_keys, d_com1, d_blinder1, d_com2, d_blinder2, C.byref(rng), d_out, out_cap, d_status))

    def link_verify_batch(self, com1, com2, proofs):
        """zk_link_verify_batch for B (com1, com2, proof) triples, every proof 256 bytes.  Returns (ok list, status list)."""
        B = len(proofs)
        size = self.link_proof_size()
        if any(len(p) != size for p in proofs):
            raise ValueError('a link proof is %d bytes' % size)
        ok = (C.c_uint8 * max(B, 1))()
        st = (C.c_int32 * max(B, 1))()
        self._chk(self.L.zk_link_verify_batch(self.h, B, self._rows(com1, 72, B, 'com1'), self._rows(com2, 72, B, 'com2'), b''.join(proofs) if B else bytes(size), ok, st))
        return list(ok)[:B], list(st)[:B]

    def link_verify_batch_device(self, B, d_com1, d_com2, d_proofs, d_ok, d_status):
        self._chk(self.L.zk_link_verify_batch_device(self.h, B, d_com1, d_com2, d_proofs, d_ok, d_status))

    def proof_key_commitments(self, proofs, offsets=None):
        """zk_proof_key_commitments: keyXcom of every ZKA1 / ZK1P proof (the context's wire layout) as a 72-byte Tom-256 point.  proofs: a list of byte strings,
        or one blob with `offsets` (B + 1 entries).  Returns (coms, statuses); a refused slot gives 72 zero bytes and status 10."""
        if offsets is None:
            blob, offsets, o = b''.join(proofs), [], 0
            for p in proofs:
                offsets.append(o)
                o += len(p)
            offsets.append(o)
        else:
            blob = bytes(proofs)
        B = len(offsets) - 1
        off = (C.c_uint64 * (B + 1))(*offsets)
        com = C.create_string_buffer(max(72 * B, 1))
        st = (C.c_int32 * max(B, 1))()
        self._chk(self.L.zk_proof_key_commitments(self.h, B, blob if blob else bytes(4), off, com, st))
        return [com.raw[72 * b:72 * b + 72] for b in range(B)], list(st)[:B]

    def proof_key_commitments_device(self, B, d_proofs, d_off, d_com, d_status):
        self._chk(self.L.zk_proof_key_commitments_device(self.h, B, d_proofs, d_off, d_com, d_status))

    # ---- distinct-key proofs (zk_distinct_*): two Tom-256 commitments hide DIFFERENT keys ("ZKD1", 744 bytes)
    def distinct_proof_size(self):
        return int(self.L.zk_distinct_proof_size())

    @staticmethod
    def distinct_pairs(k):
        """the k (k - 1) / 2 pairs (i, j), i < j, of k commitments in lexicographic order: one distinct-key proof per pair shows k different keys"""
        return [(i, j) for i in range(k) for j in range(i + 1, k)]

    def distinct_prove_batch(self, key1, com1, blinder1, key2, com2, blinder2, seeds=None, streams=None, stream_blocks=0, cap=None):
        """zk_distinct_prove_batch: proof b shows that com1[b] = key1[b] g + blinder1[b] h and com2[b] = key2[b] g + blinder2[b] h hide different keys; it
        verifies for (com1, com2) in this order only.  keys, blinders: 32-byte big-endian scalars (a list, or B x 32 bytes), coms: 72-byte Tom-256 points.
        seeds / streams must be FRESH: never the ones either commitment's proof was made with.  Returns (proofs: list of 744-byte strings, None where the
        status is not 0; statuses); equal keys give status 14.  self.distinct_last_raw keeps the B slots as the call wrote them (a slot whose status is
        not 0 is zero-filled), and cap overrides the out_cap handed to the call (default 744 B; a smaller one makes the call refuse with ZK_E_BUFFER)."""
        B = len(key1) // 32 if isinstance(key1, (bytes, bytearray, memoryview)) else len(key1)
        k1, c1, b1 = self._rows(key1, 32, B, 'key1'), self._rows(com1, 72, B, 'com1'), self._rows(blinder1, 32, B, 'blinder1')
        k2, c2, b2 = self._rows(key2, 32, B, 'key2'), self._rows(com2, 72, B, 'com2'), self._rows(blinder2, 32, B, 'blinder2')
        if seeds is None and streams is None:
            seeds = os.urandom(32 * B)
        rng, _keep = self._rng(B, seeds, streams, stream_blocks)
        size = self.distinct_proof_size()
        out = C.create_string_buffer(max(size * B, 1))
        st = (C.c_int32 * max(B, 1))()
        self._chk(self.L.zk_distinct_prove_batch(self.h, B, k1, c1, b1, k2, c2, b2, C.byref(rng), out, size * B if cap is None else cap, st))
        raw = out.raw
        self.distinct_last_raw = raw[:size * B]
        return [raw[size * b:size * (b + 1)] if st[b] == 0 else None for b in range(B)], list(st)[:B]

    def distinct_prove_batch_device(self, B, d_key1, d_com1, d_blinder1, d_key2, d_com2, d_blinder2, d_rng, d_out, out_cap, d_status, mode=0, stride_blocks=0):
        rng = ZkRng(mode, d_rng, stride_blocks)
        self._chk(self.L.zk_distinct_prove_batch_device(self.h, B, d_key1, d_com1, d_blinder1, d_key2, d_com2, d_blinder2, C.byref(rng), d_out, out_cap, d_status))

    def distinct_verify_batch(self, com1, com2, proofs):
        """zk_distinct_verify_batch for B (com1, com2, proof) triples, every proof 744 bytes.  Returns (ok list, status list)."""
        B = len(proofs)
        size = self.distinct_proof_size()
        if any(len(p) != size for p in proofs):
            raise ValueError('a distinct-key proof is %d bytes' % size)
        ok = (C.c_uint8 * max(B, 1))()
        st = (C.c_int32 * max(B, 1))()
        self._chk(self.L.zk_distinct_verify_batch(self.h, B, self._rows(com1, 72, B, 'com1'), self._rows(com2, 72, B, 'com2'), b''.join(proofs) if B else bytes(size), ok, st))
        return list(ok)[:B], list(st)[:B]

    def distinct_verify_batch_device(self, B, d_com1, d_com2, d_proofs, d_ok, d_status):
        self._chk(self.L.zk_distinct_verify_batch_device(self.h, B, d_com1, d_com2, d_proofs, d_ok, d_status))

    # ---- quorum proofs (zk_quorum_*): k attestations by k different ring members as one "ZKQ1" bundle
    def quorum_pair_count(self, k):
        """zk_quorum_pair_count: k (k - 1) / 2, 0 for a k outside 2..16"""
        return int(self.L.zk_quorum_pair_count(k))

    def quorum_proof_max_size(self, k):
        """zk_quorum_proof_max_size: upper bound of one bundle's size over the active ring (0 without params / ring or for a k outside 2..16)"""
        return int(self.L.zk_quorum_proof_max_size(self.h, k))

    def quorum_prove_batch(self, k, msg, sig, pk, which, seeds=None, pair_seeds=None, streams=None, stream_blocks=0, pair_streams=None, pair_stream_blocks=0,
                           cap=None, want_member_status=True):
        """zk_quorum_prove_batch: Q = len(which) // k quorums of k members each over the active ring; member m = q k + i uses row m of msg, sig, pk, which and
        seeds, pair p of quorum q row q P + p of pair_seeds (P = k (k - 1) / 2).  Both seed sets come from os.urandom when absent; they must be independent of
        each other.  Returns (bundles: list of byte strings, None where the quorum's status is not 0; quorum statuses; member statuses).  cap overrides the
        out_cap handed to the call."""
        n = len(which)
        if k <= 0 or n % k:
            raise ValueError('k members per quorum')
        Q, P = n // k, k * (k - 1) // 2
        if seeds is None and streams is None:
            seeds = os.urandom(32 * n)
        if pair_seeds is None and pair_streams is None:
            pair_seeds = os.urandom(32 * Q * P)
        rng, _keep = self._rng(n, seeds, streams, stream_blocks)
        rng_pairs, _keep2 = self._rng(Q * P, pair_seeds, pair_streams, pair_stream_blocks)
        size = max(self.quorum_proof_max_size(k) * Q, 16)
        out = C.create_string_buffer(size)
        off = (C.c_uint64 * (Q + 1))()
        st = (C.c_int32 * max(Q, 1))()
        mst = (C.c_int32 * max(n, 1))()
        w = (C.c_uint32 * max(n, 1))(*which)
        self._chk(self.L.zk_quorum_prove_batch(self.h, Q, k, bytes(msg), bytes(sig), bytes(pk), w, C.byref(rng), C.byref(rng_pairs), out, size if cap is None else cap, off, st,
                                               mst if want_member_status else None))
        raw = out.raw
        return [raw[off[q]:off[q + 1]] if st[q] == 0 else None for q in range(Q)], list(st)[:Q], list(mst)[:n] if want_member_status else None

    def quorum_prove_batch_device(self, Q, k, d_msg, d_sig, d_pk, d_which, d_rng, d_rng_pairs, d_out, out_cap, d_out_off, d_status, d_member_status=None, mode=0, stride_blocks=0,
                                  pair_mode=0, pair_stride_blocks=0):
        rng, rng_pairs = ZkRng(mode, d_rng, stride_blocks), ZkRng(pair_mode, d_rng_pairs, pair_stride_blocks)
        self._chk(self.L.zk_quorum_prove_batch_device(self.h, Q, k, d_msg, d_sig, d_pk, d_which, C.byref(rng), C.byref(rng_pairs), d_out, out_cap, d_out_off, d_status,
                                                      d_member_status))

    def quorum_verify_batch(self, k, msg, bundles, vseeds=None, want_first_bad=True):
        """zk_quorum_verify_batch: bundle q against rows q k .. q k + k - 1 of msg.  Returns (ok list, status list, first_bad list): first_bad names the first
        element that failed -- a member (< k) or a pair (k + p) -- and is 0xFFFFFFFF where ok is 1."""
        Q = len(bundles)
        off = (C.c_uint64 * (Q + 1))()
        for q, b in enumerate(bundles):
            off[q + 1] = off[q] + len(b)
        ok = (C.c_uint8 * max(Q, 1))()
        st = (C.c_int32 * max(Q, 1))()
        bad = (C.c_uint32 * max(Q, 1))()
        self._chk(self.L.zk_quorum_verify_batch(self.h, Q, k, bytes(msg), b''.join(bundles) if Q else bytes(16), off, None if vseeds is None else bytes(vseeds), ok, st,
                                                bad if want_first_bad else None))
        return list(ok)[:Q], list(st)[:Q], list(bad)[:Q] if want_first_bad else None

    def quorum_verify_batch_device(self, Q, k, d_msg, d_bundles, d_bundle_off, d_vseeds, d_ok, d_status, d_first_bad=None):
        self._chk(self.L.zk_quorum_verify_batch_device(self.h, Q, k, d_msg, d_bundles, d_bundle_off, d_vseeds, d_ok, d_status, d_first_bad))

    # ---- quorum proofs over several rings (zk_rings_quorum_*): one resident ring id per member; the wire format is ZKQ1 unchanged
    def quorum_proof_max_size_rings(self, k, ring_ids):
        """zk_rings_quorum_proof_max_size: upper bound of one bundle's size when member i proves over ring ring_ids[i] (0 for a k outside 2..16 or an id that is
        not resident)"""
        if len(ring_ids) != k:
            raise ValueError('one ring id per member')
        return int(self.L.zk_rings_quorum_proof_max_size(self.h, k, (C.c_uint32 * max(k, 1))(*ring_ids)))

    def quorum_prove_batch_rings(self, k, msg, sig, pk, which, ring_ids, seeds=None, pair_seeds=None, streams=None, stream_blocks=0, pair_streams=None,
                                 pair_stream_blocks=0, cap=None, want_member_status=True):
        """zk_rings_quorum_prove_batch: quorum_prove_batch with member m proving over resident ring ring_ids[m] (which[m] indexes that ring); the active ring is
        neither read nor changed.  Returns (bundles, quorum statuses, member statuses) like quorum_prove_batch."""
        n = len(which)
        if k <= 0 or n % k or len(ring_ids) != n:
            raise ValueError('k members per quorum, one ring id per member')
        Q, P = n // k, k * (k - 1) // 2
        if seeds is None and streams is None:
            seeds = os.urandom(32 * n)
        if pair_seeds is None and pair_streams is None:
            pair_seeds = os.urandom(32 * Q * P)
        rng, _keep = self._rng(n, seeds, streams, stream_blocks)
        rng_pairs, _keep2 = self._rng(Q * P, pair_seeds, pair_streams, pair_stream_blocks)
        sizes = {r: self.ring_proof_max_size(r) for r in set(ring_ids)}
        size = max(sum(sizes[r] for r in ring_ids) + Q * (16 + 744 * P), 16)   # the exact capacity rule: an id that is not resident counts 0
        out = C.create_string_buffer(size)
        off = (C.c_uint64 * (Q + 1))()
        st = (C.c_int32 * max(Q, 1))()
        mst = (C.c_int32 * max(n, 1))()
        w = (C.c_uint32 * max(n, 1))(*which)
        ids = (C.c_uint32 * max(n, 1))(*ring_ids)
        self._chk(self.L.zk_rings_quorum_prove_batch(self.h, Q, k, bytes(msg), bytes(sig), bytes(pk), w, ids, C.byref(rng), C.byref(rng_pairs), out,
                                                     size if cap is None else cap, off, st, mst if want_member_status else None))
        raw = out.raw
        return [raw[off[q]:off[q + 1]] if st[q] == 0 else None for q in range(Q)], list(st)[:Q], list(mst)[:n] if want_member_status else None

    def quorum_prove_batch_rings_device(self, Q, k, d_msg, d_sig, d_pk, d_which, d_ids, d_rng, d_rng_pairs, d_out, out_cap, d_out_off, d_status, d_member_status=None, mode=0,
                                        stride_blocks=0, pair_mode=0, pair_stride_blocks=0):
        rng, rng_pairs = ZkRng(mode, d_rng, stride_blocks), ZkRng(pair_mode, d_rng_pairs, pair_stride_blocks)
        self._chk(self.L.zk_rings_quorum_prove_batch_device(self.h, Q, k, d_msg, d_sig, d_pk, d_which, d_ids, C.byref(rng), C.byref(rng_pairs), d_out, out_cap, d_out_off,
                                                            d_status, d_member_status))

    def quorum_verify_batch_rings(self, k, msg, bundles, ring_ids, verifier_seeds=None, want_first_bad=True):
        """zk_rings_quorum_verify_batch: quorum_verify_batch with member m verified over resident ring ring_ids[m].  Returns (ok, statuses, first_bad)."""
        Q = len(bundles)
        if len(ring_ids) != Q * k:
            raise ValueError('one ring id per member')
        off = (C.c_uint64 * (Q + 1))()
        for q, b in enumerate(bundles):
            off[q + 1] = off[q] + len(b)
        ok = (C.c_uint8 * max(Q, 1))()
        st = (C.c_int32 * max(Q, 1))()
        bad = (C.c_uint32 * max(Q, 1))()
        ids = (C.c_uint32 * max(Q * k, 1))(*ring_ids)
        self._chk(self.L.zk_rings_quorum_verify_batch(self.h, Q, k, bytes(msg), b''.join(bundles) if Q else bytes(16), off, ids,
                                                      None if verifier_seeds is None else bytes(verifier_seeds), ok, st, bad if want_first_bad else None))
        return list(ok)[:Q], list(st)[:Q], list(bad)[:Q] if want_first_bad else None

    def quorum_verify_batch_rings_device(self, Q, k, d_msg, d_bundles, d_bundle_off, d_ids, d_vseeds, d_ok, d_status, d_first_bad=None):
        self._chk(self.L.zk_rings_quorum_verify_batch_device(self.h, Q, k, d_msg, d_bundles, d_bundle_off, d_ids, d_vseeds, d_ok, d_status, d_first_bad))

    # ---- escrow tags (zk_ctx_set_auditor, zk_escrow_*): ElGamal of a committed key under an auditor's key, tied to the commitment ("ZKT1", 472 bytes)
    def set_auditor(self, auditor_xy72):
        """zk_ctx_set_auditor: the auditor's public key A (72 bytes) for the escrow calls; zk_ctx_set_params drops it"""
        if len(auditor_xy72) != 72:
            raise ValueError('the auditor key is a 72-byte Tom-256 point')
        self._chk(self.L.zk_ctx_set_auditor(self.h, bytes(auditor_xy72)))

    def escrow_keygen(self, secret_be32):
        """zk_escrow_keygen: A = a g for the 32-byte big-endian secret a (reduced mod q; 0 is refused)"""
        if len(secret_be32) != 32:
            raise ValueError('the secret is 32 bytes')
        out = C.create_string_buffer(72)
        self._chk(self.L.zk_escrow_keygen(self.h, bytes(secret_be32), out))
        return out.raw

    def escrow_tag_size(self):
        return int(self.L.zk_escrow_tag_size())

    def escrow_prove_batch(self, keys, com, blinder, seeds=None, streams=None, stream_blocks=0, cap=None):
        """zk_escrow_prove_batch: tag b encrypts keys[b] under the context's auditor key and shows that it is the key of com[b] = keys[b] g + blinder[b] h.
        keys, blinders: 32-byte big-endian scalars (a list, or B x 32 bytes), com: 72-byte Tom-256 points.  seeds / streams must be FRESH: never the ones
        the commitment's proof was made with.  Returns (tags: list of 472-byte strings, None where the status is not 0; statuses).  self.escrow_last_raw keeps
        the B slots as the call wrote them, and cap overrides the out_cap handed to the call, as link_prove_batch has them."""
        B = len(keys) // 32 if isinstance(keys, (bytes, bytearray, memoryview)) else len(keys)
        k, c1, b1 = self._rows(keys, 32, B, 'keys'), self._rows(com, 72, B, 'com'), self._rows(blinder, 32, B, 'blinder')
        if seeds is None and streams is None:
            seeds = os.urandom(32 * B)
        rng, _keep = self._rng(B, seeds, streams, stream_blocks)
        size = self.escrow_tag_size()
        out = C.create_string_buffer(max(size * B, 1))
        st = (C.c_int32 * max(B, 1))()
        self._chk(self.L.zk_escrow_prove_batch(self.h, B, k, c1, b1, C.byref(rng), out, size * B if cap is None else cap, st))
        raw = out.raw
        self.escrow_last_raw = raw[:size * B]
        return [raw[size * b:size * (b + 1)] if st[b] == 0 else None for b in range(B)], list(st)[:B]

    def escrow_prove_batch_device(self, B, d_keys, d_com, d_blinder, d_rng, d_out, out_cap, d_status, mode=0, stride_blocks=0):
        rng = ZkRng(mode, d_rng, stride_blocks)
        self._chk(self.L.zk_escrow_prove_batch_device(self.h, B, d_keys, d_com, d_blinder, C.byref(rng), d_out, out_cap, d_status))

    def escrow_verify_batch(self, com, tags):
        """zk_escrow_verify_batch for B (com, tag) pairs, every tag 472 bytes.  Returns (ok list, status list)."""
        B = len(tags)
        size = self.escrow_tag_size()
        if any(len(t) != size for t in tags):
            raise ValueError('an escrow tag is %d bytes' % size)
        ok = (C.c_uint8 * max(B, 1))()
        st = (C.c_int32 * max(B, 1))()
        self._chk(self.L.zk_escrow_verify_batch(self.h, B, self._rows(com, 72, B, 'com'), b''.join(tags) if B else bytes(size), ok, st))
        return list(ok)[:B], list(st)[:B]

    def escrow_verify_batch_device(self, B, d_com, d_tags, d_ok, d_status):
        self._chk(self.L.zk_escrow_verify_batch_device(self.h, B, d_com, d_tags, d_ok, d_status))

    def escrow_open_batch(self, secret_be32, tags):
        """zk_escrow_open_batch: the auditor's call against the active ring.  Returns (indices: the lowest ring index whose key the tag carries, 0xffffffff
        for none; statuses).  It does not verify: call escrow_verify_batch first."""
        B = len(tags)
        size = self.escrow_tag_size()
        if len(secret_be32) != 32 or any(len(t) != size for t in tags):
            raise ValueError('the secret is 32 bytes and an escrow tag %d' % size)
        idx = (C.c_uint32 * max(B, 1))()
        st = (C.c_int32 * max(B, 1))()
        self._chk(self.L.zk_escrow_open_batch(self.h, B, bytes(secret_be32), b''.join(tags) if B else bytes(size), idx, st))
        return list(idx)[:B], list(st)[:B]

    def escrow_open_batch_device(self, B, d_secret, d_tags, d_index, d_status):
        self._chk(self.L.zk_escrow_open_batch_device(self.h, B, d_secret, d_tags, d_index, d_status))

    def escrow_open_batch_rings(self, secret_be32, tags, ring_ids):
        """zk_rings_escrow_open_batch: the auditor's call with one resident ring id per tag (ESCROW_RING_ANY: every resident ring, ascending ids); the active
        ring is not involved.  Returns (rings: the id of the ring that holds the tag's key, indices: its lowest index there -- both 0xffffffff for none --,
        statuses).  It does not verify: call escrow_verify_batch first."""
        B = len(tags)
        size = self.escrow_tag_size()
        if len(secret_be32) != 32 or any(len(t) != size for t in tags) or len(ring_ids) != B:
            raise ValueError('the secret is 32 bytes, an escrow tag %d, and every tag has a ring id' % size)
        ids = (C.c_uint32 * max(B, 1))(*ring_ids)
        ring, idx = (C.c_uint32 * max(B, 1))(), (C.c_uint32 * max(B, 1))()
        st = (C.c_int32 * max(B, 1))()
        self._chk(self.L.zk_rings_escrow_open_batch(self.h, B, bytes(secret_be32), b''.join(tags) if B else bytes(size), ids, ring, idx, st))
        return list(ring)[:B], list(idx)[:B], list(st)[:B]

    def escrow_open_batch_rings_device(self, B, d_secret, d_tags, d_ring_ids, d_ring_out, d_index, d_status):
        self._chk(self.L.zk_rings_escrow_open_batch_device(self.h, B, d_secret, d_tags, d_ring_ids, d_ring_out, d_index, d_status))

    # ---- accountable attestations (zk_accountable_*): an attestation and the escrow tag of its keyXcom as one "ZKC1" bundle
    def accountable_proof_max_size(self):
        """zk_accountable_proof_max_size: 16 + proof_max_size + 472 (0 without params / an active ring)"""
        return int(self.L.zk_accountable_proof_max_size(self.h))

    @staticmethod
    def _slots(blobs):
        off = (C.c_uint64 * (len(blobs) + 1))()
        for b, x in enumerate(blobs):
            off[b + 1] = off[b] + len(x)
        return off

    def accountable_prove_batch(self, msg, sig, pk, which, seeds=None, tag_seeds=None, streams=None, stream_blocks=0, tag_streams=None, tag_stream_blocks=0, cap=None,
                                want_part_status=True):
        """zk_accountable_prove_batch: B = len(which) bundles over the active ring under the context's auditor key; bundle b uses row b of every array.  Both
        seed sets come from os.urandom when absent; they must be independent of each other.  Returns (bundles: list of byte strings, None where the status is
        not 0; statuses; part statuses: B (attestation, tag) pairs).  self.accountable_last_raw keeps (bytes, offsets) as the call wrote them; cap overrides the
        out_cap handed to the call."""
        B = len(which)
        if seeds is None and streams is None:
            seeds = os.urandom(32 * B)
        if tag_seeds is None and tag_streams is None:
            tag_seeds = os.urandom(32 * B)
        rng, _keep = self._rng(B, seeds, streams, stream_blocks)
        rng_tags, _keep2 = self._rng(B, tag_seeds, tag_streams, tag_stream_blocks)
        size = max(self.accountable_proof_max_size() * B, 16)
        out = C.create_string_buffer(size)
        off = (C.c_uint64 * (B + 1))()
        st = (C.c_int32 * max(B, 1))()
        pst = (C.c_int32 * max(2 * B, 1))()
        w = (C.c_uint32 * max(B, 1))(*which)
        self._chk(self.L.zk_accountable_prove_batch(self.h, B, bytes(msg), bytes(sig), bytes(pk), w, C.byref(rng), C.byref(rng_tags), out, size if cap is None else cap, off, st,
                                                    pst if want_part_status else None))
        raw = out.raw
        self.accountable_last_raw = (raw[:off[B]], list(off))
        return ([raw[off[b]:off[b + 1]] if st[b] == 0 else None for b in range(B)], list(st)[:B],
                [(pst[2 * b], pst[2 * b + 1]) for b in range(B)] if want_part_status else None)

    def accountable_prove_batch_device(self, B, d_msg, d_sig, d_pk, d_which, d_rng, d_rng_tags, d_out, out_cap, d_out_off, d_status, d_part_status=None, mode=0, stride_blocks=0,
                                       tag_mode=0, tag_stride_blocks=0):
        rng, rng_tags = ZkRng(mode, d_rng, stride_blocks), ZkRng(tag_mode, d_rng_tags, tag_stride_blocks)
        self._chk(self.L.zk_accountable_prove_batch_device(self.h, B, d_msg, d_sig, d_pk, d_which, C.byref(rng), C.byref(rng_tags), d_out, out_cap, d_out_off, d_status,
                                                           d_part_status))

    def accountable_verify_batch(self, msg, bundles, vseeds=None, want_first_bad=True, blob=None, offsets=None):
        """zk_accountable_verify_batch: bundle b against row b of msg.  bundles: a list of byte strings, or one blob with offsets (B + 1 entries).  Returns (ok
        list, status list, first_bad list): first_bad is 0 for the attestation, 1 for the tag and 0xFFFFFFFF where ok is 1."""
        if blob is None:
            blob, off = b''.join(bundles), self._slots(bundles)
        else:
            off = (C.c_uint64 * len(offsets))(*offsets)
        B = len(off) - 1
        ok = (C.c_uint8 * max(B, 1))()
        st = (C.c_int32 * max(B, 1))()
        bad = (C.c_uint32 * max(B, 1))()
        self._chk(self.L.zk_accountable_verify_batch(self.h, B, bytes(msg), bytes(blob) if len(blob) else bytes(16), off, None if vseeds is None else bytes(vseeds), ok, st,
                                                     bad if want_first_bad else None))
        return list(ok)[:B], list(st)[:B], list(bad)[:B] if want_first_bad else None

    def accountable_verify_batch_device(self, B, d_msg, d_bundles, d_bundle_off, d_vseeds, d_ok, d_status, d_first_bad=None):
        self._chk(self.L.zk_accountable_verify_batch_device(self.h, B, d_msg, d_bundles, d_bundle_off, d_vseeds, d_ok, d_status, d_first_bad))

    def accountable_split(self, bundles, cap=None, blob=None, offsets=None):
        """zk_accountable_split_batch: pure layout.  Returns (attestations: list of byte strings, b'' for a refused bundle; tags: list of 472-byte strings, zero
        bytes for a refused bundle; statuses).  self.accountable_last_raw keeps the attestations' (bytes, offsets) as the call wrote them."""
        if blob is None:
            blob, off = b''.join(bundles), self._slots(bundles)
        else:
            off = (C.c_uint64 * len(offsets))(*offsets)
        B = len(off) - 1
        size = max(len(blob), 16)
        att = C.create_string_buffer(size)
        aoff = (C.c_uint64 * (B + 1))()
        tags = C.create_string_buffer(max(472 * B, 1))
        st = (C.c_int32 * max(B, 1))()
        self._chk(self.L.zk_accountable_split_batch(self.h, B, bytes(blob) if len(blob) else bytes(16), off, att, size if cap is None else cap, aoff, tags, st))
        raw, traw = att.raw, tags.raw
        self.accountable_last_raw = (raw[:aoff[B]], list(aoff))
        return [raw[aoff[b]:aoff[b + 1]] for b in range(B)], [traw[472 * b:472 * b + 472] for b in range(B)], list(st)[:B]

    def accountable_split_device(self, B, d_bundles, d_bundle_off, d_att_out, att_cap, d_att_off, d_tags_out, d_status):
        self._chk(self.L.zk_accountable_split_batch_device(self.h, B, d_bundles, d_bundle_off, d_att_out, att_cap, d_att_off, d_tags_out, d_status))

    def accountable_join(self, proofs, tags, cap=None):
        """zk_accountable_join_batch: pure layout.  Returns (bundles: list of byte strings, None where join refuses; statuses)."""
        B = len(proofs)
        if len(tags) != B or any(len(t) != 472 for t in tags):
            raise ValueError('one 472-byte tag per proof')
        off = self._slots(proofs)
        size = max(off[B] + 488 * B, 16)
        out = C.create_string_buffer(size)
        ooff = (C.c_uint64 * (B + 1))()
        st = (C.c_int32 * max(B, 1))()
        self._chk(self.L.zk_accountable_join_batch(self.h, B, b''.join(proofs) if off[B] else bytes(16), off, b''.join(tags) if B else bytes(472), out, size if cap is None else cap,
                                                   ooff, st))
        raw = out.raw
        self.accountable_last_raw = (raw[:ooff[B]], list(ooff))
        return [raw[ooff[b]:ooff[b + 1]] if st[b] == 0 else None for b in range(B)], list(st)[:B]

    def accountable_join_device(self, B, d_proofs, d_proof_off, d_tags, d_out, out_cap, d_out_off, d_status):
        self._chk(self.L.zk_accountable_join_batch_device(self.h, B, d_proofs, d_proof_off, d_tags, d_out, out_cap, d_out_off, d_status))

    # ---- accountable attestations over several rings (zk_rings_accountable_*): one resident ring id per bundle, no active ring; the wire format is ZKC1 unchanged
    def ring_accountable_proof_max_size(self, ring):
        """zk_rings_accountable_proof_max_size: 16 + ring_proof_max_size(ring) + 472 (0 for an id that is not resident / without params)"""
        return int(self.L.zk_rings_accountable_proof_max_size(self.h, ring))

    def accountable_prove_batch_rings(self, msg, sig, pk, which, ring_ids, seeds=None, tag_seeds=None, streams=None, stream_blocks=0, tag_streams=None, tag_stream_blocks=0,
                                      cap=None, want_part_status=True, fill=None):
        """zk_rings_accountable_prove_batch: accountable_prove_batch with bundle b proving over resident ring ring_ids[b] (which[b] indexes that ring); the active
        ring is neither read nor changed.  The buffer handed to the call has exactly the capacity rule's size (an id that is not resident counts 0); cap
        overrides the out_cap handed to the call; fill (one byte value) pre-fills every output, and self.accountable_last_outputs keeps them all as the call
        left them (bytes, offsets, statuses, part statuses).  Returns (bundles, statuses, part statuses) like accountable_prove_batch."""
        B = len(which)
        if len(ring_ids) != B:
            raise ValueError('one ring id per proof')
        if seeds is None and streams is None:
            seeds = os.urandom(32 * B)
        if tag_seeds is None and tag_streams is None:
            tag_seeds = os.urandom(32 * B)
        rng, _keep = self._rng(B, seeds, streams, stream_blocks)
        rng_tags, _keep2 = self._rng(B, tag_seeds, tag_streams, tag_stream_blocks)
        sizes = {r: self.ring_accountable_proof_max_size(r) for r in set(ring_ids)}
        exact = sum(sizes[r] for r in ring_ids)
        out = C.create_string_buffer(max(exact, 16))
        off = (C.c_uint64 * (B + 1))()
        st = (C.c_int32 * max(B, 1))()
        pst = (C.c_int32 * max(2 * B, 1))()
        if fill is not None:
            C.memset(out, fill, len(out)), C.memset(off, fill, C.sizeof(off)), C.memset(st, fill, C.sizeof(st)), C.memset(pst, fill, C.sizeof(pst))
        w = (C.c_uint32 * max(B, 1))(*which)
        ids = (C.c_uint32 * max(B, 1))(*ring_ids)
        rc = self.L.zk_rings_accountable_prove_batch(self.h, B, bytes(msg), bytes(sig), bytes(pk), w, ids, C.byref(rng), C.byref(rng_tags), out, exact if cap is None else cap, off,
                                                     st, pst if want_part_status else None)
        self.accountable_last_outputs = (out.raw, list(off), list(st), list(pst))
        self._chk(rc)
        raw = out.raw
        self.accountable_last_raw = (raw[:off[B]], list(off))
        return ([raw[off[b]:off[b + 1]] if st[b] == 0 else None for b in range(B)], list(st)[:B],
                [(pst[2 * b], pst[2 * b + 1]) for b in range(B)] if want_part_status else None)

    def accountable_prove_batch_rings_device(self, B, d_msg, d_sig, d_pk, d_which, d_ring_ids, d_rng, d_rng_tags, d_out, out_cap, d_out_off, d_status, d_part_status=None, mode=0,
                                             stride_blocks=0, tag_mode=0, tag_stride_blocks=0):
        rng, rng_tags = ZkRng(mode, d_rng, stride_blocks), ZkRng(tag_mode, d_rng_tags, tag_stride_blocks)
        self._chk(self.L.zk_rings_accountable_prove_batch_device(self.h, B, d_msg, d_sig, d_pk, d_which, d_ring_ids, C.byref(rng), C.byref(rng_tags), d_out, out_cap, d_out_off,
                                                                 d_status, d_part_status))

    def accountable_verify_batch_rings(self, msg, bundles, ring_ids, vseeds=None, want_first_bad=True, blob=None, offsets=None):
        """zk_rings_accountable_verify_batch: accountable_verify_batch with bundle b's attestation verified over resident ring ring_ids[b].  Returns (ok list,
        status list, first_bad list)."""
        if blob is None:
            blob, off = b''.join(bundles), self._slots(bundles)
        else:
            off = (C.c_uint64 * len(offsets))(*offsets)
        B = len(off) - 1
        if len(ring_ids) != B:
            raise ValueError('one ring id per proof')
        ok = (C.c_uint8 * max(B, 1))()
        st = (C.c_int32 * max(B, 1))()
        bad = (C.c_uint32 * max(B, 1))()
        ids = (C.c_uint32 * max(B, 1))(*ring_ids)
        self._chk(self.L.zk_rings_accountable_verify_batch(self.h, B, bytes(msg), bytes(blob) if len(blob) else bytes(16), off, ids, None if vseeds is None else bytes(vseeds),
                                                           ok, st, bad if want_first_bad else None))
        return list(ok)[:B], list(st)[:B], list(bad)[:B] if want_first_bad else None

    def accountable_verify_batch_rings_device(self, B, d_msg, d_bundles, d_bundle_off, d_ring_ids, d_vseeds, d_ok, d_status, d_first_bad=None):
        self._chk(self.L.zk_rings_accountable_verify_batch_device(self.h, B, d_msg, d_bundles, d_bundle_off, d_ring_ids, d_vseeds, d_ok, d_status, d_first_bad))

    def accountable_open_batch_rings(self, secret_be32, bundles, ring_ids, fill=None, blob=None, offsets=None):
        """zk_rings_accountable_open_batch: the auditor's call on bundles, one resident ring id per bundle (ESCROW_RING_ANY: every resident ring, ascending
        ids).  Returns (rings, indices -- both 0xffffffff for none --, statuses) like escrow_open_batch_rings.  fill pre-fills the three outputs, and
        self.accountable_last_outputs keeps them as the call left them.  It does not verify: call accountable_verify_batch_rings first."""
        if blob is None:
            blob, off = b''.join(bundles), self._slots(bundles)
        else:
            off = (C.c_uint64 * len(offsets))(*offsets)
        B = len(off) - 1
        if len(secret_be32) != 32 or len(ring_ids) != B:
            raise ValueError('the secret is 32 bytes, and every bundle has a ring id')
        ids = (C.c_uint32 * max(B, 1))(*ring_ids)
        ring, idx = (C.c_uint32 * max(B, 1))(), (C.c_uint32 * max(B, 1))()
        st = (C.c_int32 * max(B, 1))()
        if fill is not None:
            C.memset(ring, fill, C.sizeof(ring)), C.memset(idx, fill, C.sizeof(idx)), C.memset(st, fill, C.sizeof(st))
        rc = self.L.zk_rings_accountable_open_batch(self.h, B, bytes(secret_be32), bytes(blob) if len(blob) else bytes(16), off, ids, ring, idx, st)
        self.accountable_last_outputs = (list(ring), list(idx), list(st))
        self._chk(rc)
        return list(ring)[:B], list(idx)[:B], list(st)[:B]

    def accountable_open_batch_rings_device(self, B, d_secret, d_bundles, d_bundle_off, d_ring_ids, d_ring_out, d_index, d_status):
        self._chk(self.L.zk_rings_accountable_open_batch_device(self.h, B, d_secret, d_bundles, d_bundle_off, d_ring_ids, d_ring_out, d_index, d_status))

    # ---- threshold opening (zk_ctx_set_auditors, zk_auditors_*): t of n auditors open a tag through verifiable shares ("ZKS1", 264 bytes)
    def auditors_share_size(self):
        return int(self.L.zk_auditors_share_size())

    def auditors_split_key(self, secret_be32, t, n, seed=None, stream=None, stream_blocks=0):
        """zk_auditors_split_key: the dealer's Shamir split of the auditor secret a.  Returns (shares: n 32-byte scalars a_j = f(j); keys: n 72-byte points
        A_j = a_j g).  seed: 32 bytes (fresh; os.urandom where neither is given), or stream: stream_blocks 32-byte blocks."""
        if len(secret_be32) != 32:
            raise ValueError('the secret is 32 bytes')
        if seed is None and stream is None:
            seed = os.urandom(32)
        rng, _keep = self._rng(1, seed, stream, stream_blocks)
        shares, keys = C.create_string_buffer(32 * 16), C.create_string_buffer(72 * 16)
        self._chk(self.L.zk_auditors_split_key(self.h, bytes(secret_be32), t, n, C.byref(rng), shares, keys))
        return [shares.raw[32 * j:32 * j + 32] for j in range(n)], [keys.raw[72 * j:72 * j + 72] for j in range(n)]

    def set_auditors(self, t, keys):
        """zk_ctx_set_auditors: the share keys A_1 .. A_n (72 bytes each) of a t-of-n opening; they must interpolate to the context's auditor key"""
        n = len(keys)
        if any(len(k) != 72 for k in keys):
            raise ValueError('a share key is a 72-byte Tom-256 point')
        self._chk(self.L.zk_ctx_set_auditors(self.h, t, n, b''.join(bytes(k) for k in keys) if n else bytes(72)))

    def _escrow_tags_blob(self, tags):
        size = self.escrow_tag_size()
        if any(len(t) != size for t in tags):
            raise ValueError('an escrow tag is %d bytes' % size)
        return b''.join(tags) if tags else bytes(size)

    def auditors_share_batch(self, j, share_secret_be32, tags, seeds=None, streams=None, stream_blocks=0, cap=None):
        """zk_auditors_share_batch: auditor j's shares of the tags.  Returns (shares: list of 264-byte strings, None where the status is not 0; statuses).
        self.share_last_raw keeps the B slots as the call wrote them, and cap overrides the out_cap handed to the call, as escrow_prove_batch has them."""
        B = len(tags)
        if len(share_secret_be32) != 32:
            raise ValueError('the share secret is 32 bytes')
        if seeds is None and streams is None:
            seeds = os.urandom(32 * B)
        rng, _keep = self._rng(B, seeds, streams, stream_blocks)
        size = self.auditors_share_size()
        out = C.create_string_buffer(max(size * B, 1))
        st = (C.c_int32 * max(B, 1))()
        self._chk(self.L.zk_auditors_share_batch(self.h, B, j, bytes(share_secret_be32), self._escrow_tags_blob(tags), C.byref(rng), out, size * B if cap is None else cap, st))
        raw = out.raw
        self.share_last_raw = raw[:size * B]
        return [raw[size * b:size * (b + 1)] if st[b] == 0 else None for b in range(B)], list(st)[:B]

    def auditors_share_batch_device(self, B, j, d_share_secret, d_tags, d_rng, d_out, out_cap, d_status, mode=0, stride_blocks=0):
        rng = ZkRng(mode, d_rng, stride_blocks)
        self._chk(self.L.zk_auditors_share_batch_device(self.h, B, j, d_share_secret, d_tags, C.byref(rng), d_out, out_cap, d_status))

    def auditors_share_verify_batch(self, tags, shares):
        """zk_auditors_share_verify_batch for B (tag, share) pairs; the auditor's index comes from each share's header.  Returns (ok list, status list)."""
        B = len(tags)
        size = self.auditors_share_size()
        if len(shares) != B or any(len(s) != size for s in shares):
            raise ValueError('every tag has one share of %d bytes' % size)
        ok = (C.c_uint8 * max(B, 1))()
        st = (C.c_int32 * max(B, 1))()
        self._chk(self.L.zk_auditors_share_verify_batch(self.h, B, self._escrow_tags_blob(tags), b''.join(shares) if B else bytes(size), ok, st))
        return list(ok)[:B], list(st)[:B]

    def auditors_share_verify_batch_device(self, B, d_tags, d_shares, d_ok, d_status):
        self._chk(self.L.zk_auditors_share_verify_batch_device(self.h, B, d_tags, d_shares, d_ok, d_status))

    def auditors_combine_batch(self, auditors, tags, shares, ring_ids, t=None):
        """zk_auditors_combine_batch: shares[s][b] is auditor auditors[s]'s share of tags[b]; one resident ring id (or ESCROW_RING_ANY) per tag.  Returns
        (rings, indices -- both 0xffffffff for none --, statuses) as escrow_open_batch_rings does.  It does not verify: call auditors_share_verify_batch first."""
        B = len(tags)
        t = len(auditors) if t is None else t
        size = self.auditors_share_size()
        if len(shares) != len(auditors) or any(len(row) != B or any(len(s) != size for s in row) for row in shares) or len(ring_ids) != B:
            raise ValueError('one row of B %d-byte shares per auditor, and every tag has a ring id' % size)
        aud = (C.c_uint32 * max(len(auditors), 1))(*auditors)
        ids = (C.c_uint32 * max(B, 1))(*ring_ids)
        ring, idx = (C.c_uint32 * max(B, 1))(), (C.c_uint32 * max(B, 1))()
        st = (C.c_int32 * max(B, 1))()
        self._chk(self.L.zk_auditors_combine_batch(self.h, B, t, aud, self._escrow_tags_blob(tags), b''.join(b''.join(row) for row in shares) if B else bytes(size), ids, ring, idx, st))
        return list(ring)[:B], list(idx)[:B], list(st)[:B]

    def auditors_combine_batch_device(self, B, t, d_auditors, d_tags, d_shares, d_ring_ids, d_ring_out, d_index, d_status):
        self._chk(self.L.zk_auditors_combine_batch_device(self.h, B, t, d_auditors, d_tags, d_shares, d_ring_ids, d_ring_out, d_index, d_status))

    def synth_params(self, seed):
        a, b, c = C.create_string_buffer(64), C.create_string_buffer(72), C.create_string_buffer(72)
        self._chk(self.L.zk_synth_params(self.h, seed, a, b, c))
        return a.raw, b.raw, c.raw

    def synth_workload(self, seed, nkeys, B):
        ring = C.create_string_buffer(32 * nkeys)
        msg, sig, pk = C.create_string_buffer(32 * max(B, 1)), C.create_string_buffer(64 * max(B, 1)), C.create_string_buffer(64 * max(B, 1))
        which = (C.c_uint32 * max(B, 1))()
        seeds = C.create_string_buffer(32 * max(B, 1))
        self._chk(self.L.zk_synth_workload(self.h, seed, nkeys, B, ring, msg, sig, pk, which, seeds))
        return ring.raw, msg.raw[:32 * B], sig.raw[:64 * B], pk.raw[:64 * B], list(which)[:B], seeds.raw[:32 * B]

    def last_timing(self):
        total = C.c_float()
        names = (C.c_char_p * 32)()
        ms = (C.c_float * 32)()
        n = self.L.zk_last_timing(self.h, C.byref(total), names, ms, 32)
        return total.value, {names[i].decode(): ms[i] for i in range(min(n, 32))}

    def set_timing(self, mode):
        """zk_ctx_set_timing: 0 never, 1 per-family events in every blocking call, 2 (default) only in calls of more than 8 192 proofs"""
        self.L.zk_ctx_set_timing.argtypes = [C.c_void_p, C.c_int]
        self.L.zk_ctx_set_timing.restype = C.c_int
        self._chk(self.L.zk_ctx_set_timing(self.h, int(mode)))

    def last_wall_ms(self):
        """earliest start -> latest end of the last call's timed kernel families (last_timing()[0] is their sum, which overlapping families exceed)"""
        self.L.zk_last_wall_ms.argtypes = [C.c_void_p]
        self.L.zk_last_wall_ms.restype = C.c_float
        return float(self.L.zk_last_wall_ms(self.h))

    # ---- unit-test hooks
    def test_field_op(self, which, op, a_list, b_list):
        n = len(a_list)
        a = b''.join(x.to_bytes(40, 'big') for x in a_list)
        b = b''.join(x.to_bytes(40, 'big') for x in b_list)
        out = C.create_string_buffer(40 * n)
        self._chk(self.L.zk_test_field_op(self.h, which, op, n, a, b, out))
        return [int.from_bytes(out.raw[40 * i:40 * i + 40], 'big') for i in range(n)]

    def test_tom_commit(self, v_list, r_list):
        n = len(v_list)
        out = C.create_string_buffer(72 * n)
        self._chk(self.L.zk_test_tom_commit(self.h, n, b''.join(x.to_bytes(32, 'big') for x in v_list),
                                            b''.join(x.to_bytes(32, 'big') for x in r_list), out))
        return [out.raw[72 * i:72 * i + 72] for i in range(n)]

    def test_tom_commit_shape(self, shape, v_list, r_list):
        """zk_test_tom_commit_shape: the commitments through one named kernel (1 one lane, 2 list B with its pairs, 3 four lanes, 4 cooperating waves, 5 compacted list)"""
        n = len(v_list)
        out = C.create_string_buffer(72 * n)
        self._chk(self.L.zk_test_tom_commit_shape(self.h, shape, n, b''.join(x.to_bytes(32, 'big') for x in v_list),
                                                  b''.join(x.to_bytes(32, 'big') for x in r_list), out))
        return [out.raw[72 * i:72 * i + 72] for i in range(n)]

    def test_p256_fixed_mul(self, base_sel, k_list):
        n = len(k_list)
        out = C.create_string_buffer(64 * n)
        self._chk(self.L.zk_test_p256_fixed_mul(self.h, base_sel, n, b''.join(x.to_bytes(32, 'big') for x in k_list), out))
        return [out.raw[64 * i:64 * i + 64] for i in range(n)]

    def test_exp_sum(self, key, neg, gkb_list):
        """zk_test_exp_sum: for every (g, k, b) the sums T = g G + k (+- ring key `key`), A = T + b h of the Exp commit phase's key-table kernel.  Returns
        (T, A, T_complete, A_complete, fell): four lists of 64-byte affine points (zero bytes: the identity) and the fallback flags (bit 0: T, bit 1: A)."""
        n = len(gkb_list)
        out = C.create_string_buffer(256 * n)
        fell = (C.c_uint32 * n)()
        self._chk(self.L.zk_test_exp_sum(self.h, key, 1 if neg else 0, n, b''.join(x.to_bytes(32, 'big') for t in gkb_list for x in t), out, fell))
        cols = [[out.raw[64 * (c * n + i):64 * (c * n + i) + 64] for i in range(n)] for c in range(4)]
        return cols[0], cols[1], cols[2], cols[3], list(fell)

    @staticmethod
    def _in_ptr(buf, nbytes):
        """bytes or a C-contiguous numpy array of exactly nbytes -> what a void * argument takes (the caller keeps `buf` alive)"""
        if isinstance(buf, (bytes, bytearray)):
            assert len(buf) == nbytes, (len(buf), nbytes)
            return bytes(buf)
        assert buf.flags['C_CONTIGUOUS'] and buf.nbytes == nbytes, (buf.nbytes, nbytes)
        return buf.ctypes.data

    def test_msm_sum(self, groups, cap_proofs, count, nq, table, term_idx, term_sc, coef):
        """zk_test_msm_sum: the Tom-256 cross-proof bucket pass on caller-chosen terms.  table: 72-byte affine points; term_idx (uint32) and term_sc (32 bytes
        big-endian each) per term id of the cap_proofs * (720 + 8 nq + 3) term slots (bytes or numpy arrays); coef: count x (mg, mh, eg, eh) as ints or 128 count
        bytes.  Returns (tw, one, flags, live, oversized): tw[w][grp] and one[grp] 72-byte affine points (zero bytes: the identity)."""
        nw = 20 if groups == 64 else 16
        nt = cap_proofs * (720 + 8 * nq + 3)
        tab = b''.join(table)
        if not isinstance(coef, (bytes, bytearray)):
            coef = b''.join(x.to_bytes(32, 'big') for t in coef for x in t)
        assert len(tab) == 72 * len(table) and len(coef) == 128 * count
        tw, one = C.create_string_buffer(72 * nw * groups), C.create_string_buffer(72 * groups)
        flags, cnt = (C.c_uint32 * groups)(), (C.c_uint32 * 2)()
        self._chk(self.L.zk_test_msm_sum(self.h, groups, cap_proofs, count, nq, len(table), tab, self._in_ptr(term_idx, 4 * nt), self._in_ptr(term_sc, 32 * nt),
                                         bytes(coef) if count else None, tw, one, flags, cnt))
        tw = [[tw.raw[72 * (w * groups + g):72 * (w * groups + g) + 72] for g in range(groups)] for w in range(nw)]
        return tw, [one.raw[72 * g:72 * g + 72] for g in range(groups)], list(flags), cnt[0], cnt[1]

    def test_pmsm_sum(self, groups, cap_proofs, count, table, term_idx, term_sc):
        """zk_test_pmsm_sum: the P-256 cross-proof pass (pack, group, bucket, reduce) on caller-chosen terms.  table: 64-byte affine points; term ids 20 p + j
        for the A terms, 20 cap_proofs + p for the Clambda terms.  Returns (tw, flags, beyond, oversized): tw[w][grp] = sum_d d B_d as 64-byte affine points
        (zero bytes: the identity), the pass's verdicts, counters[1] and counters[2]."""
        nw = 14 if groups == 64 else 11
        nt = cap_proofs * 21
        tab = b''.join(table)
        assert len(tab) == 64 * len(table)
        tw = C.create_string_buffer(64 * nw * groups)
        flags, cnt = (C.c_uint32 * groups)(), (C.c_uint32 * 2)()
        self._chk(self.L.zk_test_pmsm_sum(self.h, groups, cap_proofs, count, len(table), tab, self._in_ptr(term_idx, 4 * nt), self._in_ptr(term_sc, 32 * nt), tw, flags, cnt))
        tw = [[tw.raw[64 * (w * groups + g):64 * (w * groups + g) + 64] for g in range(groups)] for w in range(nw)]
        return tw, list(flags), cnt[0], cnt[1]

    def test_sha256(self, msgs):
        n, ln = len(msgs), len(msgs[0])
        assert all(len(m) == ln for m in msgs)
        out = C.create_string_buffer(32 * n)
        self._chk(self.L.zk_test_sha256(self.h, n, ln, b''.join(msgs), out))
        return [out.raw[32 * i:32 * i + 32] for i in range(n)]

    def test_rng_draws(self, B, first_k, n_k, seeds=None, streams=None, stream_blocks=0):
        if streams is None:
            data = C.create_string_buffer(bytes(seeds), 32 * B)
            rng = ZkRng(0, C.cast(data, C.c_void_p), 0)
        else:
            data = C.create_string_buffer(bytes(streams), 32 * B * stream_blocks)
            rng = ZkRng(1, C.cast(data, C.c_void_p), stream_blocks)
        out = C.create_string_buffer(32 * B * n_k)
        self._chk(self.L.zk_test_rng_draws(self.h, B, C.byref(rng), first_k, n_k, out))
        return [[out.raw[32 * (b * n_k + j):32 * (b * n_k + j) + 32] for j in range(n_k)] for b in range(B)]


class Pool:
    """Several GPUs of one node behind one handle (zk_pool, include/zkattest.h): the batch is split into contiguous shards, the
    ring is uploaded once and broadcast device-to-device (RCCL over xGMI, peer copies as fallback)."""

    def __init__(self, device_ids):
        self.L = lib()
        ids = (C.c_int * len(device_ids))(*device_ids)
        h = C.c_void_p()
        rc = self.L.zk_pool_create(ids, len(device_ids), C.byref(h))
        self.h = h
        self._chk(rc)
        self.n = len(device_ids)

    def _chk(self, rc):
        if rc:
            raise ZkError(rc, self.L.zk_pool_last_error(self.h).decode())   # NULL handle: why zk_pool_create failed

    def close(self):
        if getattr(self, 'h', None):
            self.L.zk_pool_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        """zk_pool_last_error: after set_ring also why RCCL was not used"""
        return self.L.zk_pool_last_error(self.h).decode()

    def rccl_library(self):
        """zk_pool_rccl_library: the file the nccl* entry points came from ('' while RCCL was never loaded)"""
        return self.L.zk_pool_rccl_library(self.h).decode()

    def engine(self, i):
        """Per-device context (settings only: chunk, lanes, comb width, host taper); owned by the pool."""
        return Engine(_borrowed=self.L.zk_pool_ctx(self.h, i))

    def numa_node(self, i):
        return self.L.zk_pool_numa_node(self.h, i)

    def shard_ms(self):
        ms = (C.c_float * self.n)()
        self.L.zk_pool_shard_ms(self.h, ms, self.n)
        return [round(float(x), 2) for x in ms]

    def shard(self, B, i):
        f, c = C.c_uint64(), C.c_uint64()
        self.L.zk_pool_shard(self.h, B, i, C.byref(f), C.byref(c))
        return f.value, c.value

    def set_params(self, nist_h64, tom_g72, tom_h72, sec_level=80):
        self._chk(self.L.zk_pool_set_params(self.h, bytes(nist_h64), bytes(tom_g72), bytes(tom_h72), sec_level))

    def set_verify_level(self, per_proof):
        """zk_pool_set_verify_level: Engine.set_verify_level on every shard context."""
        self._chk(self.L.zk_pool_set_verify_level(self.h, 1 if per_proof else 0))

    def set_verify_reps(self, all):
        """zk_pool_set_verify_reps: Engine.set_verify_reps on every shard context."""
        self._chk(self.L.zk_pool_set_verify_reps(self.h, 1 if all else 0))

    def set_ring(self, keys_be32, nkeys=None):
        keys_be32 = bytes(keys_be32)
        self._chk(self.L.zk_pool_set_ring(self.h, keys_be32, nkeys if nkeys is not None else len(keys_be32) // 32))
        return self.L.zk_pool_ring_transport(self.h).decode()

    def add_ring(self, keys_be32, nkeys=None):
        """zk_pool_add_ring: the same resident ring (and id) on every shard context."""
        keys_be32 = bytes(keys_be32)
        rid = C.c_uint32()
        self._chk(self.L.zk_pool_add_ring(self.h, keys_be32, nkeys if nkeys is not None else len(keys_be32) // 32, C.byref(rid)))
        return rid.value

    def use_ring(self, ring):
        self._chk(self.L.zk_pool_use_ring(self.h, ring))

    def drop_ring(self, ring):
        self._chk(self.L.zk_pool_drop_ring(self.h, ring))

    def ring_info(self, ring):
        return self.engine(0).ring_info(ring)

    def update_ring(self, ring, changes, nkeys=None):
        """zk_pool_update_ring: Engine.update_ring on every shard context."""
        cnt, idx, keys = _ring_changes(changes)
        if nkeys is None:
            nkeys = self.ring_info(ring)['n_keys']
        self._chk(self.L.zk_pool_update_ring(self.h, ring, cnt, idx, keys, nkeys))

    def verify_batch_rings(self, msg, proofs, ring_ids, vseeds=None):
        """zk_pool_verify_batch_rings: verify_batch with one resident ring id per proof, sharded by contiguous ranges."""
        B = len(proofs)
        off, ln = (C.c_uint64 * B)(), (C.c_uint64 * B)()
        o = 0
        for b, p in enumerate(proofs):
            off[b], ln[b] = o, len(p)
            o += len(p)
        blob = (C.c_uint8 * max(o, 1)).from_buffer_copy(b''.join(proofs) or b'\0')
        ids = (C.c_uint32 * max(B, 1))(*ring_ids)
        ok, st = (C.c_uint8 * B)(), (C.c_int32 * B)()
        self._chk(self.L.zk_pool_verify_batch_rings(self.h, B, bytes(msg), C.addressof(blob), off, ln, ids, bytes(vseeds) if vseeds is not None else None, ok, st))
        return list(ok), list(st)

    def prove_batch_rings(self, msg, sig, pk, which, ring_ids, seeds=None):
        """zk_pool_prove_batch_rings: prove_batch with one resident ring id per proof (ids of add_ring), sharded by contiguous ranges."""
        B = len(which)
        if len(ring_ids) != B:
            raise ValueError('one ring id per proof')
        if seeds is None:
            seeds = os.urandom(32 * B)
        per = self.engine(0)._rings_cap(1, ring_ids)
        cap = (per * (B // self.n + 1) + 256) * self.n
        out = (C.c_uint8 * cap)()
        off, ln, st = (C.c_uint64 * B)(), (C.c_uint64 * B)(), (C.c_int32 * B)()
        w = (C.c_uint32 * max(B, 1))(*which)
        ids = (C.c_uint32 * max(B, 1))(*ring_ids)
        data = C.create_string_buffer(bytes(seeds), 32 * B)
        rng = ZkRng(0, C.cast(data, C.c_void_p), 0)
        self._chk(self.L.zk_pool_prove_batch_rings(self.h, B, bytes(msg), bytes(sig), bytes(pk), w, ids, C.byref(rng), C.addressof(out), cap, off, ln, st))
        raw = bytes(out)
        return [raw[off[b]:off[b] + ln[b]] if st[b] == 0 else None for b in range(B)], list(st)

    def prove_batch_raw(self, msg, sig, pk, which, seeds, out, cap):
        """zk_pool_prove_batch into `out` (PinnedBuffer or ctypes array).  Returns (seconds, off, len, status)."""
        import time
        B = len(which)
        off, ln, st = (C.c_uint64 * B)(), (C.c_uint64 * B)(), (C.c_int32 * B)()
        w = (C.c_uint32 * B)(*which)
        data = C.create_string_buffer(bytes(seeds), 32 * B)
        rng = ZkRng(0, C.cast(data, C.c_void_p), 0)
        optr = out.ptr if isinstance(out, PinnedBuffer) else C.addressof(out)
        msg, sig, pk = bytes(msg), bytes(sig), bytes(pk)
        t0 = time.time()
        self._chk(self.L.zk_pool_prove_batch(self.h, B, msg, sig, pk, w, C.byref(rng), optr, cap, off, ln, st))
        return time.time() - t0, off, ln, st

    def prove_batch_device_out(self, msg, sig, pk, which, seeds, d_out, caps):
        """zk_pool_prove_batch_device: d_out = per-device buffers from device_alloc.  Returns (seconds, off, len, status)."""
        import time
        B = len(which)
        off, ln, st = (C.c_uint64 * B)(), (C.c_uint64 * B)(), (C.c_int32 * B)()
        w = (C.c_uint32 * B)(*which)
        data = C.create_string_buffer(bytes(seeds), 32 * B)
        rng = ZkRng(0, C.cast(data, C.c_void_p), 0)
        ptrs = (C.c_void_p * self.n)(*d_out)
        cp = (C.c_uint64 * self.n)(*caps)
        msg, sig, pk = bytes(msg), bytes(sig), bytes(pk)
        t0 = time.time()
        self._chk(self.L.zk_pool_prove_batch_device(self.h, B, msg, sig, pk, w, C.byref(rng), ptrs, cp, off, ln, st))
        return time.time() - t0, off, ln, st

    def device_alloc(self, i, nbytes):
        p = self.L.zk_pool_device_alloc(self.h, i, nbytes)
        if not p:
            raise MemoryError('zk_pool_device_alloc(%d, %d) failed' % (i, nbytes))
        return p

    def device_free(self, i, p):
        self.L.zk_pool_device_free(self.h, i, p)

    # ---- streamed pool calls: tickets keep every buffer of the job alive until its wait
    def prove_submit(self, msg, sig, pk, which, seeds, out, cap):
        B = len(which)
        t = {'B': B, 'out': out, 'off': (C.c_uint64 * B)(), 'ln': (C.c_uint64 * B)(), 'st': (C.c_int32 * B)(), 'w': (C.c_uint32 * B)(*which),
             'data': C.create_string_buffer(bytes(seeds), 32 * B), 'msg': bytes(msg), 'sig': bytes(sig), 'pk': bytes(pk), 'job': C.c_void_p()}
        t['rng'] = ZkRng(0, C.cast(t['data'], C.c_void_p), 0)
        self._chk(self.L.zk_pool_prove_submit(self.h, B, t['msg'], t['sig'], t['pk'], t['w'], C.byref(t['rng']), out.ptr, cap, t['off'], t['ln'], t['st'], C.byref(t['job'])))
        return t

    def prove_wait(self, t):
        self._chk(self.L.zk_pool_prove_wait(self.h, t['job']))
        return t['off'], t['ln'], t['st']

    def test_fail_submit(self, slot):
        """fault injection (tests): the next streamed submit of this pool fails at device slot `slot` after the earlier slots were submitted.  Only the test
        build of the library has the entry point (csrc/Makefile `testhooks`: lib/libzkattest_hip_testhooks.so, selected with ZKATTEST_LIB)."""
        if not hasattr(self.L, 'zk_test_pool_fail_next_submit'):
            raise RuntimeError('this build has no fault injection (load lib/libzkattest_hip_testhooks.so through ZKATTEST_LIB)')
        self.L.zk_test_pool_fail_next_submit.argtypes = [C.c_void_p, C.c_int]
        self.L.zk_test_pool_fail_next_submit.restype = None
        self.L.zk_test_pool_fail_next_submit(self.h, int(slot))

    def verify_submit(self, msg, proofs, off, ln, B, vseeds=None):
        t = {'B': B, 'proofs': proofs, 'off': off, 'ln': ln, 'ok': (C.c_uint8 * B)(), 'st': (C.c_int32 * B)(), 'msg': bytes(msg),
             'seeds': bytes(vseeds) if vseeds is not None else None, 'job': C.c_void_p()}
        self._chk(self.L.zk_pool_verify_submit(self.h, B, t['msg'], proofs.ptr, off, ln, t['seeds'], t['ok'], t['st'], C.byref(t['job'])))
        return t

    def verify_wait(self, t):
        self._chk(self.L.zk_pool_verify_wait(self.h, t['job']))
        return t['ok'], t['st']

    def prove_batch(self, msg, sig, pk, which, seeds=None):
        B = len(which)
        if seeds is None:
            seeds = os.urandom(32 * B)
        e = self.engine(0)
        cap = (e.proof_max_size() * (B // self.n + 1) + 256) * self.n
        out = (C.c_uint8 * cap)()
        _, off, ln, st = self.prove_batch_raw(msg, sig, pk, which, seeds, out, cap)
        raw = bytes(out)
        return [raw[off[b]:off[b] + ln[b]] if st[b] == 0 else None for b in range(B)], list(st)

    def verify_batch_raw(self, msg, proofs, off, ln, B, vseeds=None):
        import time
        ok, st = (C.c_uint8 * B)(), (C.c_int32 * B)()
        ptr = proofs.ptr if isinstance(proofs, PinnedBuffer) else C.addressof(proofs)
        msg = bytes(msg)
        t0 = time.time()
        self._chk(self.L.zk_pool_verify_batch(self.h, B, msg, ptr, off, ln, bytes(vseeds) if vseeds is not None else None, ok, st))
        return time.time() - t0, ok, st

    def verify_batch(self, msg, proofs, vseeds=None):
        B = len(proofs)
        off, ln = (C.c_uint64 * B)(), (C.c_uint64 * B)()
        o = 0
        for b, p in enumerate(proofs):
            off[b], ln[b] = o, len(p)
            o += len(p)
        blob = (C.c_uint8 * max(o, 1)).from_buffer_copy(b''.join(proofs) or b'\0')
        _, ok, st = self.verify_batch_raw(msg, blob, off, ln, B, vseeds)
        return list(ok), list(st)
