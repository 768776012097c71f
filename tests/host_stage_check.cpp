/*
 * host_stage_check.cpp -- the staged-stream layout and the chunk cut of pg_cryogen_amd/csrc/host_stage.h against brute force.  A
 * program of its own that includes that header alone: tests/test_host_stage_cpu.py builds it under -fsanitize=address,undefined
 * and expects exit 0 and one line.  The brute-force side steps byte by byte and block by block; it uses none of the header's
 * formulas.
 *
 *   layout   m in 1..40 and 700 streams of sizes 0..70 (every third one empty) and a few large ones, whole calls and subsets given
 *            by an index list: o_off 0, the tables back to back, o_data the first multiple of 64 behind them; every offset 16-byte
 *            aligned and at or after o_data; the streams ascending and apart; an empty stream takes no room; total the sum of the
 *            padded sizes (64-bit: two streams of 4 GiB - 1); the filled tables say the same, in a buffer that ends with them
 *   chunks   max_chunk_in is the largest sum of padded sizes over the chunks of a cut, chunk by chunk (700 streams: two chunks)
 *   cut      n in {1, 127, 128, 576, 577, 1152, 1153, 1200} at 16 KiB, a few n at 4 KiB, 128 KiB and 1 MiB, and blocks above 8 MiB
 *            (K = 64 up to 512 of them): K is the least multiple of 64 that holds an eighth of the call and 8 MiB + 1 block; the chunks tile 0..n,
 *            every one but the last holds K blocks; 1200 x 16 KiB is 576 / 576 / 48
 *   launch   kernels per chunk only for LZ4 decode with 512 blocks or more per chunk
 */
#include "host_stage.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s (m %zu n %zu block %zu)\n", __FILE__, __LINE__, #c, m, n, block); exit(1); } } while (0)

static size_t m, n, block; /* what the failing case was */

static uint64_t round_up_stepwise(uint64_t v, uint64_t a)
{
    while (v % a) v++;
    return v;
}

/* the layout of the streams idx[0..m) of a call whose sizes are `size` */
static void check_layout(const std::vector<uint32_t> &size, const std::vector<size_t> &idx, size_t block_cut)
{
    m = idx.size();
    const auto size_of = [&](size_t k) { return size[idx[k]]; };
    const cryo::StreamLayout L(m, size_of);
    CHECK(L.m == m && L.o_off == 0 && L.o_sz == 8 * m);
    CHECK(L.o_data == round_up_stepwise(12 * m, 64));
    uint64_t want_total = 0, end_of_last = L.o_data;
    for (size_t k = 0; k < m; k++) {
        const uint64_t off = L.offset(k);
        CHECK(off % 16 == 0 && off >= L.o_data);
        CHECK(off >= end_of_last);                         /* ascending, and apart from every stream before */
        CHECK(off == L.o_data + want_total);               /* packed: only the padding lies between two streams */
        CHECK(L.pos[k] == want_total);
        if (size_of(k) == 0) CHECK(L.pos[k + 1] == L.pos[k]); /* no room */
        end_of_last = off + size_of(k);
        want_total += round_up_stepwise(size_of(k), 16);
    }
    CHECK(L.total == want_total && L.pos[m] == want_total && L.bytes() == L.o_data + want_total);
    CHECK(end_of_last <= L.bytes());
    for (size_t a = 0; a <= m; a += 3)
        for (size_t b = a; b <= m; b += 5) {
            uint64_t sum = 0;
            for (size_t k = a; k < b; k++) sum += round_up_stepwise(size_of(k), 16);
            CHECK(L.span(a, b) == sum);
        }
    /* the tables, in a buffer that ends where they end (the sanitizer watches beyond it) */
    std::vector<uint32_t> tables(3 * m + 1, 0xa5a5a5a5u);
    L.fill_tables((uint8_t *)tables.data(), size_of);
    for (size_t k = 0; k < m; k++) {
        CHECK((tables[2 * k] | (uint64_t)tables[2 * k + 1] << 32) == L.offset(k)); /* little-endian, as the device reads it */
        CHECK(tables[2 * m + k] == size_of(k));
    }
    CHECK(tables[3 * m] == 0xa5a5a5a5u); /* nothing behind the tables */
    /* the most a chunk of a cut of these m streams brings in */
    n = m; block = block_cut;
    const cryo::ChunkCut cut(m, block_cut);
    uint64_t most = 0;
    for (size_t lo = 0; lo < m; lo += cut.K) {
        uint64_t sum = 0;
        for (size_t k = lo; k < lo + cut.K && k < m; k++) sum += round_up_stepwise(size_of(k), 16);
        if (sum > most) most = sum;
    }
    CHECK(L.max_chunk_in(cut) == most);
}

static void check_cut(size_t n_, size_t block_)
{
    n = n_; block = block_; m = 0;
    const cryo::ChunkCut cut(n, block);
    /* the least multiple of 64 that holds an eighth of the call and 8 MiB + 1 block */
    size_t eighth = 0, floor_blocks = 0, K = 64;
    while (eighth * 8 < n) eighth++;
    while ((floor_blocks + 1) * block <= ((size_t)8 << 20)) floor_blocks++;
    while (K < eighth || K < floor_blocks + 1) K += 64;
    CHECK(cut.n == n && cut.K == K && cut.K % 64 == 0);
    size_t next = 0, chunks = 0;
    for (size_t ch = 0; ch < cut.chunks(); ch++, chunks++) {
        CHECK(cut.lo(ch) == next && cut.hi(ch) > cut.lo(ch) && cut.hi(ch) <= n);
        CHECK(cut.cnt(ch) == cut.hi(ch) - cut.lo(ch));
        CHECK(ch + 1 == cut.chunks() || cut.cnt(ch) == K);
        CHECK(cut.cnt(ch) <= K);
        next = cut.hi(ch);
    }
    CHECK(next == n && chunks == cut.chunks() && chunks >= 1);
}

int main()
{
    /* sizes: small ones with every third empty, and some that span many 16-byte steps */
    std::vector<uint32_t> size(700);
    uint32_t x = 12345;
    for (size_t i = 0; i < size.size(); i++) {
        x = x * 1664525u + 1013904223u;
        size[i] = i % 3 == 2 ? 0 : i % 50 == 7 ? 4000 + (x >> 20) : (x >> 16) % 71;
    }
    for (size_t count : {(size_t)1, (size_t)2, (size_t)3, (size_t)5, (size_t)6, (size_t)16, (size_t)17, (size_t)40, (size_t)700}) {
        std::vector<size_t> all(count), every_third, backwards;
        for (size_t k = 0; k < count; k++) all[k] = k;
        for (size_t k = 1; k < count; k += 3) every_third.push_back(k);
        for (size_t k = count; k-- > 0;) if (k % 2 == 0) backwards.push_back(k);
        /* a cut with several chunks needs small blocks: K = 64 for a block above 8 MiB */
        check_layout(size, all, (size_t)9 << 20);
        check_layout(size, all, 16384);
        if (!every_third.empty()) check_layout(size, every_third, (size_t)9 << 20);
        check_layout(size, backwards, (size_t)9 << 20);
    }
    {   /* m = 1, an empty stream and a full one */
        std::vector<uint32_t> one = {0, 1, 16, 17, 0xffffffffu};
        for (size_t k = 0; k < one.size(); k++) check_layout(one, {k}, 16384);
        check_layout(one, {4, 0, 4}, 16384); /* 64-bit sums: two streams of 4 GiB - 1 */
    }
    for (size_t nn : {1, 127, 128, 576, 577, 1152, 1153, 1200}) check_cut(nn, 16384);
    for (size_t nn : {1, 2048, 2049, 4608, 16400, 16385, 100000}) check_cut(nn, 4096);
    for (size_t nn : {1, 64, 65, 512, 513, 4096, 4097}) check_cut(nn, 131072);
    for (size_t nn : {1, 9, 64, 65, 512, 513, 1000}) check_cut(nn, (size_t)1 << 20);
    for (size_t bs : {((size_t)8 << 20) + 1, (size_t)16 << 20}) {
        for (size_t nn : {1, 64, 65, 512}) check_cut(nn, bs);
        n = 512; block = bs; m = 0;
        CHECK(cryo::ChunkCut(512, bs).K == 64 && cryo::ChunkCut(512, bs).chunks() == 8);
        CHECK(cryo::ChunkCut(513, bs).K == 128);
    }
    {
        n = 1200; block = 16384; m = 0;
        const cryo::ChunkCut cut(1200, 16384);
        CHECK(cut.K == 576 && cut.chunks() == 3 && cut.cnt(0) == 576 && cut.cnt(1) == 576 && cut.cnt(2) == 48);
    }
    n = block = m = 0;
    for (int lz4 = 0; lz4 <= 1; lz4++)
        for (int encode = 0; encode <= 1; encode++) {
            CHECK(!cryo::kernel_per_chunk(511, lz4, encode));
            CHECK(cryo::kernel_per_chunk(512, lz4, encode) == (lz4 && !encode));
            CHECK(cryo::kernel_per_chunk(4096, lz4, encode) == (lz4 && !encode));
        }
    puts("host stage check ok");
    return 0;
}
