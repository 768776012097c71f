/*
 * multi_share_check.cpp -- the deal, the regions and the scatter of pg_cryogen_amd/csrc/multi_share.h against brute force.  A
 * program of its own that includes that header alone: tests/test_multi_share_cpu.py builds it under -fsanitize=address,undefined
 * and expects exit 0 and one line.  The brute-force side counts i % G block by block and walks the buffers unit by unit; it uses
 * none of the header's formulas.
 *
 *   deal     every G in 1..5, n in 0..17: the shares partition 0..n-1, each ascending; count and before are what counting i % G
 *            gives; block i is entry i / G of handle i % G; the keyed owner is key % G, or i % G for key 0
 *   regions  units of 1, 8 and 290 per block, every whole-buffer cap in 0..n * unit + 1: the regions lie in handle order and do
 *            not overlap, each holds min(want, cap - first) units or none when first >= cap, and end(0) is 0
 *   scatter  1 and 3 entries per block land where a double loop puts them and nowhere else (the output is two entries longer and
 *            filled with a sentinel); gather is its inverse
 */
#include "multi_share.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s (G %zu n %zu)\n", __FILE__, __LINE__, #c, G, n); exit(1); } } while (0)

static void check_deal(size_t G, size_t n)
{
    size_t want_count[5] = {0, 0, 0, 0, 0};
    for (size_t i = 0; i < n; i++) want_count[i % G]++;
    const cryo::RoundRobin rr{n, G};
    const std::vector<std::vector<size_t>> share = cryo::deal_shares(n, G, [&](size_t i) { return rr.handle_of(i); });
    CHECK(share.size() == G);
    std::vector<int> seen(n, 0);
    size_t want_before = 0;
    for (size_t g = 0; g < G; g++) {
        CHECK(rr.count(g) == want_count[g] && share[g].size() == want_count[g]);
        CHECK(rr.before(g) == want_before);
        want_before += want_count[g];
        for (size_t k = 0; k < share[g].size(); k++) {
            CHECK(share[g][k] < n && share[g][k] % G == g);
            CHECK(k == 0 || share[g][k] > share[g][k - 1]);
            seen[share[g][k]]++;
        }
    }
    CHECK(rr.before(G) == n);
    for (size_t i = 0; i < n; i++) {
        CHECK(seen[i] == 1);
        CHECK(rr.handle_of(i) == i % G && rr.entry_of(i) == i / G);
        CHECK(share[rr.handle_of(i)][rr.entry_of(i)] == i);
        CHECK(cryo::keyed_owner(0, i, G) == i % G);
        CHECK(cryo::keyed_owner(1000 + 7 * i, i, G) == (1000 + 7 * i) % G);
    }
    /* a deal by keys: every block with the handle its owner names, ascending */
    const std::vector<std::vector<size_t>> keyed = cryo::deal_shares(n, G, [&](size_t i) { return cryo::keyed_owner(i % 3 ? 5 * i : 0, i, G); });
    size_t dealt = 0;
    for (size_t g = 0; g < G; g++)
        for (size_t k = 0; k < keyed[g].size(); k++, dealt++) {
            const size_t i = keyed[g][k];
            CHECK(i < n && (i % 3 ? 5 * i % G : i % G) == g);
            CHECK(k == 0 || i > keyed[g][k - 1]);
        }
    CHECK(dealt == n);
}

static void check_regions(size_t G, size_t n)
{
    static const uint64_t units[3] = {1, 8, 290};
    uint64_t blocks[5] = {0, 0, 0, 0, 0}, before[5] = {0, 0, 0, 0, 0};
    for (size_t i = 0; i < n; i++) blocks[i % G]++;
    for (size_t g = 1; g < G; g++) before[g] = before[g - 1] + blocks[g - 1];
    for (uint64_t u : units) {
        uint64_t room[5] = {0, 0, 0, 0, 0}; /* the units of each region that lie below the cap, counted unit by unit as it rises */
        for (uint64_t cap = 0; cap <= n * u + 1; cap++) {
            std::vector<uint64_t> ends;
            uint64_t want_last = 0;
            for (size_t g = 0; g < G; g++) {
                const uint64_t at = before[g] * u;
                const cryo::ShareRegion r(cap, before[g], blocks[g], u);
                CHECK(r.first == at && r.cap == room[g]);
                CHECK(r.first + r.cap <= (cap > at ? cap : at));                       /* cut at the cap */
                CHECK(g + 1 == G || r.first + r.cap <= before[g + 1] * u);             /* and before the next region */
                CHECK(r.cap == blocks[g] * u || r.first + r.cap == cap || (r.cap == 0 && at >= cap));
                CHECK(r.end(0) == 0 && r.end(1) == at + 1 && r.end(r.cap) == (r.cap ? at + r.cap : 0));
                static char buf[17 * 290 * 24 + 24];
                CHECK(r.in(buf) == (room[g] ? buf + at : nullptr));
                CHECK(r.in(buf, 24) == (room[g] ? buf + at * 24 : nullptr));
                ends.push_back(r.end(g % 2 ? r.cap : 0));
                if (g % 2 && r.cap) want_last = at + r.cap; /* handle order: a later end is a larger one */
            }
            CHECK(cryo::last_end(ends) == want_last);
            for (size_t g = 0; g < G; g++) room[g] += cap >= before[g] * u && cap < (before[g] + blocks[g]) * u; /* unit `cap` */
        }
    }
    CHECK(cryo::last_end({}) == 0);
}

static void check_scatter(size_t G, size_t n)
{
    const std::vector<std::vector<size_t>> share = cryo::deal_shares(n, G, [&](size_t i) { return i % G; });
    for (size_t per = 1; per <= 3; per += 2) {
        const int SENTINEL = -1;
        std::vector<int> out(n * per + 2, SENTINEL), want(n * per + 2, SENTINEL), in(n * per + 1);
        for (size_t x = 0; x < in.size(); x++) in[x] = (int)(1000 + x);
        for (size_t g = 0; g < G; g++) {
            std::vector<int> packed(share[g].size() * per + 1);
            for (size_t x = 0; x < packed.size(); x++) packed[x] = (int)(100 * g + x);
            for (size_t k = 0; k < share[g].size(); k++)
                for (size_t j = 0; j < per; j++) want[share[g][k] * per + j] = (int)(100 * g + k * per + j);
            cryo::scatter(share[g], packed.data(), out.data(), per);
            const std::vector<int> got = cryo::gather(share[g], in.data(), per);
            CHECK(got.size() == share[g].size() * per);
            for (size_t k = 0; k < share[g].size(); k++)
                for (size_t j = 0; j < per; j++) CHECK(got[k * per + j] == (int)(1000 + share[g][k] * per + j));
        }
        CHECK(out == want);
        CHECK(out[n * per] == SENTINEL && out[n * per + 1] == SENTINEL);
        for (size_t x = 0; x < n * per; x++) CHECK(out[x] != SENTINEL);
    }
}

int main()
{
    for (size_t G = 1; G <= 5; G++)
        for (size_t n = 0; n <= 17; n++) {
            check_deal(G, n);
            check_regions(G, n);
            check_scatter(G, n);
        }
    puts("multi share check ok");
    return 0;
}
