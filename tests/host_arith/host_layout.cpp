// csrc/layout.h on the host: Carver::take and the two-pass helper lay_out, with no HIP anywhere.  A layout here is what the host layer's are -- a struct the
// layout function fills from a Carver in a fixed order -- with the regions recorded so that they can be checked: the size pass (null base) gives the real pass's
// total, every region starts on a multiple of 256 from the base, regions do not overlap, the last one ends inside what was reserved.  The buffer is a heap
// block of exactly the reserved size and every region is written end to end, so the AddressSanitizer build sees any region that leaves it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>
#include "layout.h"

struct Regions {
    std::vector<std::pair<uint8_t*, size_t>> r;
};
static size_t regions_layout(Regions& X, uint8_t* base, const std::vector<size_t>& sizes) {
    Carver k(base);
    X.r.clear();
    for (size_t s : sizes) X.r.push_back({(uint8_t*)k.take(s), s});
    return k.off + ZK_LAYOUT_TAIL;
}

static int failures = 0;
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) {                       \
            failures++;                      \
            fprintf(stderr, "FAIL %s: ", name); \
            fprintf(stderr, __VA_ARGS__);    \
            fprintf(stderr, "\n");           \
        }                                    \
    } while (0)

static void run(const char* name, const std::vector<size_t>& sizes) {
    Regions X;
    size_t sized = 0, reserved = 0, real = 0;
    int passes = 0;
    uint8_t* block = nullptr;
    const int err = lay_out(
        [&](uint8_t* base) {
            const size_t total = regions_layout(X, base, sizes);
            if (!base) {
                sized = total;
                for (auto& q : X.r) CHECK(q.first == nullptr, "the size pass handed out a pointer");
            } else real = total;
            passes++;
            return total;
        },
        [&](size_t need, uint8_t** base) {
            reserved = need;
            *base = block = (uint8_t*)malloc(need);
            return block ? 0 : 1;
        });
    CHECK(err == 0 && passes == 2, "lay_out returned %d after %d passes", err, passes);
    CHECK(sized == real && sized == reserved, "size pass %zu, reserved %zu, real pass %zu", sized, reserved, real);
    CHECK(X.r.size() == sizes.size(), "%zu regions of %zu", X.r.size(), sizes.size());
    size_t prev_end = 0;
    for (size_t i = 0; i < X.r.size(); i++) {
        const size_t at = (size_t)(X.r[i].first - block), len = X.r[i].second;
        CHECK(at % ZK_LAYOUT_ALIGN == 0, "region %zu starts at %zu", i, at);
        CHECK(at >= prev_end, "region %zu starts at %zu, inside its predecessor (ends at %zu)", i, at, prev_end);
        CHECK(at - prev_end < ZK_LAYOUT_ALIGN, "region %zu starts at %zu, a whole unit behind its predecessor's end %zu", i, at, prev_end);
        CHECK(at + len <= reserved, "region %zu ends at %zu of %zu", i, at + len, reserved);
        memset(X.r[i].first, 0xa5, len);
        prev_end = at + len;
    }
    CHECK(reserved - prev_end >= ZK_LAYOUT_TAIL && reserved - prev_end < ZK_LAYOUT_TAIL + ZK_LAYOUT_ALIGN, "tail of %zu bytes behind the last region", reserved - prev_end);
    free(block);
    printf("%-28s %2zu regions, %8zu bytes\n", name, sizes.size(), reserved);
}

int main() {
    // the shapes of the host layer's layouts (api.hip, api_verify.hip, api_member.hip), at sizes that leave every region but a few off the 256-byte grid
    const size_t B = 1000, classes = 130, Wp = 7;
    run("census of 1000", {B, 4 * ((B + 1023) / 1024) * classes, 8 * classes, 4 * B});
    run("verify window of 7", {8 * (Wp + 1), 32 * Wp, 32 * Wp, Wp, 4 * Wp});
    run("prove inputs of 3", {32 * 3, 64 * 3, 64 * 3, 4 * 3, 32 * 3, 8 * 4, 4 * 3});
    run("member inputs of 256", {4 * 256, 32 * 256, 32 * 256, 72 * 256, 32 * 256, 4 * 256});   // every size a multiple of 256
    run("zero-length regions", {0, 513, 0, 0, 1, 0});
    run("one byte", {1});
    run("nothing", {});
    {   // a reservation that fails: its error comes back and the real pass does not run
        const char* name = "failed reservation";
        Regions X;
        int passes = 0;
        const int err = lay_out([&](uint8_t* base) { return passes++, regions_layout(X, base, {100, 200}); }, [&](size_t, uint8_t**) { return 7; });
        CHECK(err == 7 && passes == 1, "lay_out returned %d after %d passes", err, passes);
    }
    if (failures) return fprintf(stderr, "%d checks failed\n", failures), 1;
    printf("layout ok\n");
    return 0;
}
