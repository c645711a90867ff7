// The byte layouts of a proof, shared by the device code (engine.h) and the host-only converters (api_json.hip).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define ZK_HD __host__ __device__
#else
#define ZK_HD
#endif
#define ZK_HDR 32
#define ZK_MAXSEC 128
// The two wire layouts of a proof (include/zkattest.h): ZKA1 pads every Tom-256 coordinate from the reference's 33 bytes to 36, ZKA1P does
// not.  Every run of Tom points in the layout has an even number of points (keyXcom keyYcom | Tx Ty | C8 C10 C11 C13 | the 6 points of a
// MultProof | A_1 A_2 | 4 n membership commitments), so point PAIRS take 132 bytes and every other field stays 4-byte aligned: 5.3 % fewer
// bytes across PCIe.  The prover's writers (k_scalar.hip) emit either; the verifier's kernels read ZKA1 only and are fed through k_v_unpack.
struct Wire {
    uint32_t tc;        // bytes per Tom coordinate: 36 | 33
    uint32_t fixed;     // header, R, comS1, keyXcom, keyYcom: 304 | 292
    uint32_t rep_head;  // A, Tx, Ty, 4 scalars: 336 | 324
    uint32_t mult;      // 6 points + 7 scalars: 656 | 620
    uint32_t eq;        // 2 points + 3 scalars: 240 | 228
    uint32_t padd;      // 4 points + 4 MultProofs + 2 EqualityProofs: 3392 | 3200
    uint32_t gk_n;      // per index bit: 4 points + 3 scalars: 384 | 360
    uint32_t magic;     // first four bytes as a little-endian word: "ZKA1" | "ZK1P"
};
#define ZK_MAGIC_ZKA1 0x31414b5au
#define ZK_MAGIC_ZKA1P 0x50314b5au
ZK_HD static inline Wire wire_make(bool packed) {
    Wire w;
    w.tc = packed ? 33 : 36;
    w.fixed = ZK_HDR + 2 * 64 + 4 * w.tc;
    w.rep_head = 64 + 4 * w.tc + 4 * 32;
    w.mult = 12 * w.tc + 7 * 32;
    w.eq = 4 * w.tc + 3 * 32;
    w.padd = 8 * w.tc + 4 * w.mult + 2 * w.eq;
    w.gk_n = 8 * w.tc + 3 * 32;
    w.magic = packed ? ZK_MAGIC_ZKA1P : ZK_MAGIC_ZKA1;
    return w;
}
ZK_HD static inline uint64_t wire_proof_size(const Wire& w, uint32_t sec, uint32_t n, uint32_t z) {
    return (uint64_t)w.fixed + (uint64_t)w.rep_head * sec + (uint64_t)w.padd * z + (uint64_t)w.gk_n * n + 32;
}
// "ZKM1" (include/zkattest.h: zk_member_*): a GKProof on its own -- 16 header bytes ("ZKM1" | total_len | n | 0), then the GKProof section of a ZKA1 proof as it is
// (4 n Tom points of 72 bytes, 3 n + 1 scalars).  Fixed per ring.
#define ZKM1_HDR 16
#define ZK_MAGIC_ZKM1 0x314d4b5au
// "ZKMB": the same bytes under the magic of a BOUND membership proof, whose challenge also hashes ring digest, caller context and com (sha256.h: GK_STMT_MEMBER)
#define ZK_MAGIC_ZKMB 0x424d4b5au
ZK_HD static inline uint64_t zkm1_size(uint32_t n) { return (uint64_t)ZKM1_HDR + 288ull * n + 32ull * (3ull * n + 1); }
// Per-proof verify levels (zk_ctx_set_verify_level): the level a proof of o1 - o0 bytes at `pr` announces, 0..ZK_MAXSEC, or ZK_LV_BAD where the
// header alone already makes it ZK_E_BAD_ENCODING in the pipeline at ANY level (short, misaligned, wrong magic, a length that is not the header's,
// secLevel above 128, n above 63, or more bytes than the largest well-formed proof of that level) -- which also bounds the bytes a level's
// window can receive.  Only the first 16 header bytes are read.
#define ZK_LV_BAD (ZK_MAXSEC + 1)
#define ZK_LV_CLASSES (ZK_MAXSEC + 2)
ZK_HD static inline uint32_t wire_level_class(const uint8_t* pr, uint64_t o0, uint64_t o1, const Wire& w) {
    if (o1 < o0 + ZK_HDR || (o0 & 3) || ((o1 - o0) & 3)) return ZK_LV_BAD;
    uint32_t h[4];
    __builtin_memcpy(h, pr, 16);
    const uint32_t total = __builtin_bswap32(h[1]), sec = __builtin_bswap32(h[2]), n = __builtin_bswap32(h[3]);
    if (h[0] != w.magic || total != o1 - o0 || sec > ZK_MAXSEC || n > 63 || total > wire_proof_size(w, sec, 63, sec)) return ZK_LV_BAD;
    return sec;
}
