// TEST HARNESS (not product code): the capacity rule of the accountable attestations over several rings (zkp-ecdsa_amd/csrc/accountable_plan.h:
// zkc_capacity_rings, zkc_capacity_add, zkc_capacity_total, zkc_capacity_fits) compiled for the host CPU with plain g++ as a program of its own, so that it
// runs under -fsanitize=address,undefined.  It reads its vectors from the file tests/test_accountable_rings_host.py writes out of a plain Python restatement,
// one per line:
//     T <count> <id resident proof_max> x count      the table of the lines that follow (at most 16 entries)
//     C <want total> <want used> <want fits 0|1> <n> <id> x n      the sum over a list of n ids, the set of entries named, whether n slots can wrap
//     M <id> <want max_size>                          one ring's zk_rings_accountable_proof_max_size
//     A <a> <b> <want>                                the saturating addition
//     F <n> <want fits 0|1>                           whether the slots of n bundles, all of the largest resident ring, stay below 2^64
// The ids lie in a heap block of exactly their size: a read outside it is the sanitizer's to report.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "accountable_plan.h"

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("usage: host_accountable_rings VECTORS\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    QuorumRings R{};
    unsigned tables = 0, sums = 0, sizes = 0, adds = 0, lineno = 0;
    while (std::getline(in, line)) {
        lineno++;
        std::istringstream ss(line);
        std::string kind;
        ss >> kind;
        if (kind == "T") {
            R = QuorumRings{};
            ss >> R.count;
            if (R.count > ZKQ_RINGS) {
                printf("line %u: a table of %u entries\n", lineno, R.count);
                return 1;
            }
            for (uint32_t r = 0; r < R.count; r++) ss >> R.id[r] >> R.resident[r] >> R.proof_max[r];
            tables++;
        } else if (kind == "C") {
            uint64_t want_total, n;
            uint32_t want_used, want_fits;
            ss >> want_total >> want_used >> want_fits >> n;
            uint32_t* ids = (uint32_t*)malloc(n ? 4 * n : 1);
            for (uint64_t i = 0; i < n; i++) ss >> ids[i];
            uint32_t used = 0;
            const uint64_t total = zkc_capacity_total(R, n, ids, &used);
            uint64_t by_hand = 0;   // the rule bundle by bundle, as a kernel lane applies it, added without the `used` set
            for (uint64_t i = 0; i < n; i++) by_hand = zkc_capacity_add(by_hand, zkc_capacity_rings(R, ids[i], nullptr));
            free(ids);
            if (total != want_total || by_hand != want_total || used != want_used || (uint32_t)zkc_capacity_fits(R, n) != want_fits) {
                printf("line %u: total %" PRIu64 " (by hand %" PRIu64 ") used %u fits %d, want %" PRIu64 " %u %u\n", lineno, total, by_hand, used, (int)zkc_capacity_fits(R, n),
                       want_total, want_used, want_fits);
                return 1;
            }
            sums++;
        } else if (kind == "M") {
            uint32_t id;
            uint64_t want;
            ss >> id >> want;
            if (zkc_capacity_rings(R, id, nullptr) != want) {
                printf("line %u: max size %" PRIu64 ", want %" PRIu64 "\n", lineno, zkc_capacity_rings(R, id, nullptr), want);
                return 1;
            }
            sizes++;
        } else if (kind == "A") {
            uint64_t a, b, want;
            ss >> a >> b >> want;
            if (zkc_capacity_add(a, b) != want) {
                printf("line %u: %" PRIu64 " + %" PRIu64 " = %" PRIu64 ", want %" PRIu64 "\n", lineno, a, b, zkc_capacity_add(a, b), want);
                return 1;
            }
            adds++;
        } else if (kind == "F") {
            uint64_t n;
            uint32_t want;
            ss >> n >> want;
            if ((uint32_t)zkc_capacity_fits(R, n) != want) {
                printf("line %u: fits %d, want %u\n", lineno, (int)zkc_capacity_fits(R, n), want);
                return 1;
            }
            adds++;
        } else if (!line.empty()) {
            printf("line %u: unknown kind\n", lineno);
            return 1;
        }
        if (ss.fail()) {
            printf("line %u: short line\n", lineno);
            return 1;
        }
    }
    if (!tables || !sums || !sizes || !adds) {
        printf("no vectors\n");
        return 1;
    }
    printf("host_accountable_rings: ok (%u tables, %u sums, %u sizes, %u additions)\n", tables, sums, sizes, adds);
    return 0;
}
