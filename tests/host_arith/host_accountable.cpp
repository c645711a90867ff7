// TEST HARNESS (not product code): the accountable attestations' plan (zkp-ecdsa_amd/csrc/accountable_plan.h: zkc_max_size, zkc_size, zkc_header,
// zkc_slot_att_bytes, zkc_walk, zkc_join_len) compiled for the host CPU with plain g++ as a program of its own, so that it runs under
// -fsanitize=address,undefined.  It reads its vectors from the file tests/test_accountable_host.py writes out of the Python statement
// (tests/accountable_common.py), one per line:
//     W <packed> <want 0|1> <o0> <o1> <att start> <tag start> <hex of the blob>      the walk of slot [o0, o1) of the blob
//     J <packed> <want length or 0> <hex of the proof> <hex of the tag>              join's length rule
//     S <proof_max> <want max_size> <att_bytes> <want size> <hex of the 16 header bytes for total = want size>
// Every blob lies in an allocation of exactly its size: a read outside it is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "accountable_plan.h"

static std::vector<uint8_t> unhex(const std::string& h) {
    std::vector<uint8_t> b(h == "-" ? 0 : h.size() / 2);
    for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)strtoul(h.substr(2 * i, 2).c_str(), nullptr, 16);
    return b;
}
// the bytes in a heap block of exactly their size (at least 1, so that the pointer is valid)
struct Exact {
    uint8_t* p;
    explicit Exact(const std::vector<uint8_t>& v) : p((uint8_t*)malloc(v.size() ? v.size() : 1)) {
        if (!v.empty()) memcpy(p, v.data(), v.size());
    }
    ~Exact() { free(p); }
};

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("usage: host_accountable VECTORS\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    unsigned walks = 0, joins = 0, sizes = 0, lineno = 0;
    while (std::getline(in, line)) {
        lineno++;
        std::istringstream ls(line);
        std::string kind;
        ls >> kind;
        bool ok = true;
        if (kind == "W") {
            int packed, want;
            uint64_t o0, o1, a0, a1;
            std::string hex;
            ls >> packed >> want >> o0 >> o1 >> a0 >> a1 >> hex;
            const std::vector<uint8_t> blob = unhex(hex);
            Exact e(blob);
            uint64_t att[2] = {~0ull, ~0ull};
            const bool got = zkc_walk(e.p, o0, o1, wire_make(packed != 0), att);
            ok = got == (want != 0) && (got ? att[0] == a0 && att[1] == a1 : att[0] == ~0ull && att[1] == ~0ull);
            ok = ok && zkc_walk(e.p, o0, o1, wire_make(packed != 0), nullptr) == got;
            if (got) ok = ok && zkc_slot_att_bytes(o0, o1) == a1 - a0;   // what the offsets alone allow is what an accepted slot holds
            walks++;
        } else if (kind == "J") {
            int packed;
            uint64_t want;
            std::string hp, ht;
            ls >> packed >> want >> hp >> ht;
            const std::vector<uint8_t> proof = unhex(hp), tag = unhex(ht);
            Exact ep(proof), et(tag);   // (a tag is always 472 bytes: join's tags are dense rows)
            ok = zkc_join_len(ep.p, 0, proof.size(), et.p, wire_make(packed != 0)) == want;
            joins++;
        } else if (kind == "S") {
            uint64_t proof_max, want_max, att, want_size;
            std::string hex;
            ls >> proof_max >> want_max >> att >> want_size >> hex;
            uint32_t hw[4];
            zkc_header(hw, (uint32_t)want_size);
            const std::vector<uint8_t> h = unhex(hex);
            ok = zkc_max_size(proof_max) == want_max && zkc_size(att) == want_size && h.size() == 16 && !memcmp(hw, h.data(), 16);
            sizes++;
        } else if (!kind.empty()) {
            ok = false;
        }
        if (!ok) {
            printf("host_accountable: FAILED line %u: %.60s\n", lineno, line.c_str());
            return 1;
        }
    }
    if (!walks || !joins || !sizes) {
        printf("host_accountable: no vectors\n");
        return 1;
    }
    printf("host_accountable: ok (%u walks, %u joins, %u sizes)\n", walks, joins, sizes);
    return 0;
}
