// csrc/sha256.h on the host: the statement writer of a bound membership proof ("ZKMB", include/zkattest.h: zk_member_*_bound) and the length / block-count
// functions the challenge hash's launch wrapper and kernels share.  For every n on the command line the program makes up 4 n points, a ring digest, a context
// and a commitment from a seeded generator, hashes  points || S_b  both ways the engine does --
//   stream: through ShaStream, as k_gk_hash and the verifier's k_v_challenges absorb it (sha_put_member_statement_head, then com as a point);
//   blocks: written out as k_gk_msg writes it (the same writer into a byte buffer, sha_put_padding over gk_hash_blocks blocks), then one compression per block --
// and prints its inputs and both digests as one line of hex per n; tests/test_member_bound_host.py rebuilds the message from the inputs and asks hashlib.
// No arguments: n = 1, 2, 3, 4, 8, 9, 12 -- 268 n + 152 bytes, i.e. 36, 48, 60, 8, 56, 4, 40 bytes into the last block: n = 3 and n = 8 spill their padding
// into a block of its own, n = 4 and n = 9 sit just behind a block boundary.
#define ZK_HOST_BUILD 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sha256.h"

static uint64_t rng_state = 0x243f6a8885a308d3ull;
static uint32_t rnd32() {   // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}
struct Coord {   // a Tom-256 coordinate as the kernels hold it before hashing: 9 little-endian words, 33 significant bytes
    uint32_t w[9];
};
static Coord coord() {
    Coord c;
    for (int i = 0; i < 8; i++) c.w[i] = rnd32();
    c.w[8] = rnd32() & 0xff;
    return c;
}
static void hex(const char* name, const uint8_t* p, size_t n) {
    printf(" %s=", name);
    for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
}
static void put_point_stream(ShaStream& s, const Coord& x, const Coord& y) {   // k_hash.hip: absorb_tom
    s.put_byte(4);
    s.put_be<33>(x.w);
    s.put_be<33>(y.w);
}
static void put_coord_bytes(uint8_t* o, const Coord& c) {   // k_hash.hip: exph_put_coord<9>
    for (int i = 0; i < 33; i++) o[i] = (uint8_t)(c.w[(32 - i) >> 2] >> (8 * ((32 - i) & 3)));
}
static int one(uint32_t n) {
    std::vector<Coord> pts(8 * n);
    for (auto& c : pts) c = coord();
    uint32_t digest[8];
    for (auto& w : digest) w = rnd32();
    uint8_t context[32];
    for (auto& b : context) b = (uint8_t)rnd32();
    const Coord cx = coord(), cy = coord();
    const uint32_t len = gk_hash_len(n, GK_STMT_MEMBER), nblk = gk_hash_blocks(n, GK_STMT_MEMBER);
    if (len != 268 * n + 152 || gk_stmt_bytes(GK_STMT_MEMBER) != 152 || gk_stmt_bytes(GK_STMT_FULL) != 220 || gk_stmt_bytes(GK_STMT_NONE) != 0) return fprintf(stderr, "n = %u: length %u\n", n, len), 1;
    if (gk_hash_len(n, GK_STMT_NONE) != 268 * n || gk_hash_len(n, GK_STMT_FULL) != 268 * n + 220) return fprintf(stderr, "n = %u: the other statements' lengths\n", n), 1;
    // ---- stream
    uint32_t lds[16], hs[8];
    ShaStream s;
    s.init(lds, 0, 1);
    for (uint32_t k = 0; k < 4 * n; k++) put_point_stream(s, pts[2 * k], pts[2 * k + 1]);
    sha_put_member_statement_head(s, digest, context);
    put_point_stream(s, cx, cy);
    if ((uint64_t)s.blocks * 64 + s.fill != len) return fprintf(stderr, "n = %u: the stream holds %llu bytes, not %u\n", n, (unsigned long long)s.blocks * 64 + s.fill, len), 1;
    s.finish(hs);
    if (s.blocks != nblk) return fprintf(stderr, "n = %u: the stream ran %u blocks, gk_hash_blocks says %u\n", n, s.blocks, nblk), 1;
    // ---- blocks: a buffer of exactly nblk blocks, guarded on both sides
    std::vector<uint8_t> buf(64 + (size_t)nblk * 64 + 64, 0xa5);
    uint8_t* m = buf.data() + 64;
    for (uint32_t k = 0; k < 4 * n; k++) m[67 * k] = 4, put_coord_bytes(m + 67 * k + 1, pts[2 * k]), put_coord_bytes(m + 67 * k + 34, pts[2 * k + 1]);
    uint32_t at = 67 * 4 * n;
    ShaBytes sink{m + at};
    sha_put_member_statement_head(sink, digest, context);
    if (sink.p != m + at + 21 + 32 + 32) return fprintf(stderr, "n = %u: the statement's head is %ld bytes\n", n, (long)(sink.p - m - at)), 1;
    at += 21 + 32 + 32;
    m[at] = 4, put_coord_bytes(m + at + 1, cx), put_coord_bytes(m + at + 34, cy);
    at += 67;
    if (at != len) return fprintf(stderr, "n = %u: wrote %u bytes\n", n, at), 1;
    sha_put_padding(m, len, nblk);
    for (size_t i = 0; i < 64; i++)
        if (buf[i] != 0xa5 || buf[64 + (size_t)nblk * 64 + i] != 0xa5) return fprintf(stderr, "n = %u: a byte outside the message's blocks was written\n", n), 1;
    uint32_t hb[8];
    sha256_iv(hb);
    for (uint32_t b = 0; b < nblk; b++) {
        uint32_t w[16];
        for (int i = 0; i < 16; i++) w[i] = (uint32_t)m[64 * b + 4 * i] << 24 | (uint32_t)m[64 * b + 4 * i + 1] << 16 | (uint32_t)m[64 * b + 4 * i + 2] << 8 | m[64 * b + 4 * i + 3];
        sha256_compress(hb, w);
    }
    // ---- the record
    printf("n=%u len=%u blocks=%u", n, len, nblk);
    std::vector<uint8_t> raw;
    for (const auto& c : pts)
        for (int i = 0; i < 33; i++) raw.push_back((uint8_t)(c.w[(32 - i) >> 2] >> (8 * ((32 - i) & 3))));
    hex("coords", raw.data(), raw.size());   // x0 y0 x1 y1 ... as 33-byte big-endian integers
    uint8_t d8[32], c66[66], out[32];
    for (int i = 0; i < 32; i++) d8[i] = (uint8_t)(digest[i >> 2] >> (24 - 8 * (i & 3)));
    hex("digest", d8, 32);
    hex("context", context, 32);
    put_coord_bytes(c66, cx), put_coord_bytes(c66 + 33, cy);
    hex("com", c66, 66);
    for (int i = 0; i < 32; i++) out[i] = (uint8_t)(hs[i >> 2] >> (24 - 8 * (i & 3)));
    hex("stream", out, 32);
    for (int i = 0; i < 32; i++) out[i] = (uint8_t)(hb[i >> 2] >> (24 - 8 * (i & 3)));
    hex("blockwise", out, 32);
    printf("\n");
    return 0;
}
int main(int argc, char** argv) {
    std::vector<uint32_t> ns = {1, 2, 3, 4, 8, 9, 12};
    if (argc > 1) {
        ns.clear();
        for (int i = 1; i < argc; i++) ns.push_back((uint32_t)atoi(argv[i]));
    }
    for (uint32_t n : ns)
        if (n < 1 || n > 63 || one(n)) return 1;
    printf("member bound hash ok\n");
    return 0;
}
