/*
 * scan_launch_check.cpp -- the host-only part of the scan calls' launch layer (pg_cryogen_amd/csrc/kernels.h), as a program
 * of its own that launches nothing: tests/test_scan_launch_cpu.py builds it with the host sanitizers and runs it.
 *
 *   routes      scan_route over truth (0 or not) x floats x like, group_route over text 0 .. 3 x buckets x the same three, against
 *               the tables written out below, which name the kernel of every route; every combination is also printed
 *               ("scan ..." / "group ..." lines) for the driver, which holds them against the docstring of
 *               tests/test_gpu_group_routes.py
 *   packing     scan_nkeys_arg for nkeys 0 .. 4 and truth 0, 1, 0x8000, 0xFFFF: the count in the low half, the table in the high
 *   grid        scan_copy_grid at cus 0, 1, 256 and cap 0, 1, 1023, 1025, against values worked out by hand
 *   predicates  filter_, agg_, group_, project_ and topn_launch_ok: one accepted argument set, then every condition violated on its
 *               own, each rejected (and what a cap of 0 excuses, accepted).  The addresses are never followed
 *   top-N pack  topn_pack on ORDER BY int4 DESC NULLS FIRST, float4 with row columns of width 1, 4, 8 at offsets 0, 4, 8 of a
 *               16-byte row:
 *                 ord_bits = column mask 0b111 << 16 | (present 1 | float 2 | float4 4) << 8 | (present 1 | nulls first 8 | desc 16)
 *                          = 0x70000 | 0x0700 | 0x19 = 0x70719
 *                 row_map  = (8 | 3 << 6) << 16 | (4 | 2 << 6) << 8 | (0 | 0 << 6) = 0xC80000 | 0x8400 | 0 = 0xC88400
 *               and its refusals: a width of 3, an offset that is no multiple of the width, a column that ends beyond the row
 */
#include <stdio.h>
#include <string.h>

#include "kernels.h"

using namespace cryo;

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("line %d: %s\n", __LINE__, #cond);                \
            failures++;                                              \
        }                                                            \
    } while (0)
/* the argument set (c, d, l) with one change: accepted or rejected by `ok` */
#define WITH(ok, want, change)                                       \
    do {                                                             \
        auto c = c0;                                                 \
        auto d = d0;                                                 \
        auto l = l0;                                                 \
        change;                                                      \
        (void)c; (void)d; (void)l;                                   \
        CHECK(ok(c, d, l) == (want));                                \
    } while (0)
#define REJECT(ok, change) WITH(ok, false, change)
#define ACCEPT(ok, change) WITH(ok, true, change)

template <class T> static T *at(uintptr_t a) { return reinterpret_cast<T *>(a); }
template <class T> static T *off(T *p, uintptr_t by) { return reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(p) + by); }
static const void *off(const void *p, uintptr_t by) { return reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(p) + by); }
static void *off(void *p, uintptr_t by) { return reinterpret_cast<void *>(reinterpret_cast<uintptr_t>(p) + by); }

/* ---- the routes ---- */
static const char *const kScanKernel[4][4] = {
    /* kRoutePlain */ {"k_filter_match<false>", "k_agg_block<false>", "k_project_block<false>", "k_topn_block<false>"},
    /* kRouteTable */ {"k_filter_match<true>", "k_agg_block<true>", "k_project_block<true>", "k_topn_block<true>"},
    /* kRouteFloat */ {"k_filterf_match", "k_aggf_block", "k_projectf_block", "k_topnf_block"},
    /* kRouteLike  */ {"k_filterl_match", "k_aggl_block", "k_projectl_block", "k_topnl_block"},
};
/* [like][floats][truth != 0] */
static const ScanRoute kScanWant[2][2][2] = {{{kRoutePlain, kRouteTable}, {kRouteFloat, kRouteFloat}}, {{kRouteLike, kRouteLike}, {kRouteLike, kRouteLike}}};

static const char *const kGroupKernel[10] = {
    /* kGroupPlain */ "k_group_block<false>", /* kGroupTable */ "k_group_block<true>", /* kGroupFloat */ "k_groupf_block",
    /* kGroupLike */ "k_groupl_block", /* kGroupBucket */ "k_groupb_block<false>", /* kGroupBucketFloat */ "k_groupb_block<true>",
    /* kGroupBucketLike */ "k_groupbl_block", /* kGroupText */ "k_groupt_block<false>", /* kGroupTextFloat */ "k_groupt_block<true>",
    /* kGroupTextLike */ "k_grouptl_block",
};
/* [0: neither, 1: buckets, 2: a text group column, buckets or not][like][floats][truth != 0] */
static const char *const kGroupWant[3][2][2][2] = {
    {{{"k_group_block<false>", "k_group_block<true>"}, {"k_groupf_block", "k_groupf_block"}},
     {{"k_groupl_block", "k_groupl_block"}, {"k_groupl_block", "k_groupl_block"}}},
    {{{"k_groupb_block<false>", "k_groupb_block<false>"}, {"k_groupb_block<true>", "k_groupb_block<true>"}},
     {{"k_groupbl_block", "k_groupbl_block"}, {"k_groupbl_block", "k_groupbl_block"}}},
    {{{"k_groupt_block<false>", "k_groupt_block<false>"}, {"k_groupt_block<true>", "k_groupt_block<true>"}},
     {{"k_grouptl_block", "k_grouptl_block"}, {"k_grouptl_block", "k_grouptl_block"}}},
};

static void check_routes()
{
    CHECK(kRoutePlain == 0 && kRouteTable == 1 && kRouteFloat == 2 && kRouteLike == 3);
    CHECK(kGroupPlain == 0 && kGroupTable == 1 && kGroupFloat == 2 && kGroupLike == 3 && kGroupBucket == 4 && kGroupBucketFloat == 5 &&
          kGroupBucketLike == 6 && kGroupText == 7 && kGroupTextFloat == 8 && kGroupTextLike == 9);
    const uint32_t truths[2] = {0u, 0x8000u};
    for (int like = 0; like < 2; like++)
        for (int floats = 0; floats < 2; floats++)
            for (int t = 0; t < 2; t++) {
                const ScanRoute r = scan_route(truths[t], floats != 0, like != 0);
                CHECK(r == kScanWant[like][floats][t]);
                printf("scan truth=%d floats=%d like=%d: %s %s %s %s\n", t, floats, like, kScanKernel[r][0], kScanKernel[r][1], kScanKernel[r][2],
                       kScanKernel[r][3]);
                for (uint32_t text = 0; text < 4u; text++)
                    for (int buckets = 0; buckets < 2; buckets++) {
                        const GroupRoute g = group_route(text, buckets != 0, truths[t], floats != 0, like != 0);
                        const char *want = kGroupWant[text ? 2 : buckets][like][floats][t];
                        CHECK((unsigned)g < 10u && strcmp(kGroupKernel[g], want) == 0);
                        printf("group text=%u buckets=%d truth=%d floats=%d like=%d: %s\n", text, buckets, t, floats, like, kGroupKernel[g]);
                    }
            }
}

/* ---- the packed argument and the grid ---- */
static void check_packing_and_grid()
{
    const uint32_t truths[4] = {0u, 1u, 0x8000u, 0xFFFFu};
    for (uint32_t nkeys = 0; nkeys <= 4u; nkeys++)
        for (uint32_t truth : truths) {
            const uint32_t a = scan_nkeys_arg(nkeys, truth);
            CHECK(a == nkeys + truth * 65536u && (a & 0xFFFFu) == nkeys && a >> 16 == truth); /* as walk_tuple takes it apart */
        }
    const int cus[3] = {0, 1, 256};
    const uint64_t caps[4] = {0u, 1u, 1023u, 1025u};
    const uint32_t want[3][4] = {{1u, 1u, 1023u, 1024u}, {1u, 1u, 4u, 4u}, {1u, 1u, 1023u, 1024u}};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) CHECK(scan_copy_grid(cus[i], caps[j]) == want[i][j]);
    CHECK(filter_side_stride(16u) == 1u && filter_side_stride(8192u) == 290u);
}

/* ---- the predicates ---- */
static ScanChunk good_chunk()
{
    ScanChunk c;
    c.d_dec = at<const uint8_t>(0x100000);
    c.dec_stride = 8192;
    c.block_size = 8192;
    c.cnt = 3;
    c.d_dec_status = at<const int32_t>(0x200000);
    return c;
}
static ScanDesc good_desc()
{
    ScanDesc d;
    d.d_atts = at<const void>(0x300004); /* 4-byte aligned is enough */
    d.d_keys = at<const void>(0x300108); /* 8-byte aligned is enough */
    d.nkeys = 4;
    d.max_att = 5;
    d.truth = 0x8000u;
    d.floats = true;
    d.like = true;
    return d;
}

/* what scan_launch_ok asks of every call alike; every call's struct has d_blocks */
template <class L> static void check_common(bool (*ok)(const ScanChunk &, const ScanDesc &, const L &), const L &l0)
{
    const ScanChunk c0 = good_chunk();
    const ScanDesc d0 = good_desc();
    ACCEPT(ok, (void)0);
    ACCEPT(ok, d.floats = d.like = false; d.truth = 0u; d.nkeys = 0u);
    ACCEPT(ok, c.block_size = 16u);
    REJECT(ok, c.dec_stride = 8200u);
    REJECT(ok, c.d_dec = off(c.d_dec, 8));
    REJECT(ok, l.d_blocks = off(l.d_blocks, 8));
    REJECT(ok, d.d_keys = off(d.d_keys, 4));
    REJECT(ok, d.d_atts = off(d.d_atts, 2));
    REJECT(ok, c.block_size = 15u);
    REJECT(ok, d.nkeys = 5u);
    REJECT(ok, d.truth = 0x10000u);
    REJECT(ok, d.like = false; d.truth = 0u); /* floats without a table */
    REJECT(ok, d.floats = false; d.truth = 0u); /* like without a table */
}

static void check_filter()
{
    FilterLaunch l0;
    l0.d_blocks = at<uint4>(0x400000);
    l0.d_side = at<uint4>(0x500000);
    l0.d_sum = at<uint64_t>(0x600000);
    l0.d_base = at<uint64_t>(0x600100);
    l0.d_running = at<uint64_t>(0x600200);
    l0.d_dst = at<uint8_t>(0x700008);
    l0.dst_cap = 1000;
    l0.d_rec = at<uint2>(0x800008);
    l0.rec_cap = 10;
    check_common(filter_launch_ok, l0);
    const ScanChunk c0 = good_chunk();
    const ScanDesc d0 = good_desc();
    REJECT(filter_launch_ok, l.d_side = off(l.d_side, 8));
    REJECT(filter_launch_ok, l.d_dst = off(l.d_dst, 4));
    REJECT(filter_launch_ok, l.d_rec = off(l.d_rec, 4));
    ACCEPT(filter_launch_ok, l.count_only = true; l.d_dst = nullptr; l.d_rec = nullptr);
}

static void check_agg()
{
    AggLaunch l0;
    l0.d_cols = at<const void>(0x300208);
    l0.ncols = 4;
    l0.d_blocks = at<uint4>(0x400000);
    l0.d_cells = at<void>(0x500008);
    check_common(agg_launch_ok, l0);
    const ScanChunk c0 = good_chunk();
    const ScanDesc d0 = good_desc();
    ACCEPT(agg_launch_ok, l.ncols = 1u);
    REJECT(agg_launch_ok, l.ncols = 0u);
    REJECT(agg_launch_ok, l.ncols = 5u);
    REJECT(agg_launch_ok, l.d_cols = off(l.d_cols, 4));
    REJECT(agg_launch_ok, l.d_cells = off(l.d_cells, 4));
}

static void check_group()
{
    GroupLaunch l0;
    l0.d_slots = at<const void>(0x300208);
    l0.nby = 2;
    l0.ncols = 4;
    l0.d_blocks = at<uint4>(0x400000);
    l0.d_side_rec = at<void>(0x500008);
    l0.d_side_cell = at<void>(0x580008);
    l0.d_running = at<uint64_t>(0x600008);
    l0.d_rec = at<void>(0x700008);
    l0.d_cells = at<void>(0x800008);
    l0.group_cap = 100;
    check_common(group_launch_ok, l0);
    const ScanChunk c0 = good_chunk();
    const ScanDesc d0 = good_desc();
    const void *buckets = at<const void>(0x300308);
    ACCEPT(group_launch_ok, l.nby = 1u; l.ncols = 0u);
    ACCEPT(group_launch_ok, d.d_buckets = buckets);
    ACCEPT(group_launch_ok, d.text = 3u);
    ACCEPT(group_launch_ok, l.nby = 1u; d.text = 1u);
    REJECT(group_launch_ok, l.nby = 0u);
    REJECT(group_launch_ok, l.nby = 3u);
    REJECT(group_launch_ok, l.ncols = 5u);
    REJECT(group_launch_ok, l.nby = 1u; d.text = 2u);                /* text >> nby != 0 */
    REJECT(group_launch_ok, d.text = 4u);
    REJECT(group_launch_ok, d.text = 1u; d.d_buckets = buckets);     /* text with buckets */
    REJECT(group_launch_ok, d.text = 1u; d.floats = d.like = false; d.truth = 0u);             /* the text kernels need a table */
    REJECT(group_launch_ok, d.d_buckets = buckets; d.floats = d.like = false; d.truth = 0u);   /* and the bucket kernels */
    REJECT(group_launch_ok, d.d_buckets = off(buckets, 4));
    REJECT(group_launch_ok, l.d_slots = off(l.d_slots, 4));
    REJECT(group_launch_ok, l.d_side_rec = off(l.d_side_rec, 4));
    REJECT(group_launch_ok, l.d_side_cell = off(l.d_side_cell, 4));
    REJECT(group_launch_ok, l.d_running = off(l.d_running, 4));
    REJECT(group_launch_ok, l.d_rec = off(l.d_rec, 4));
    REJECT(group_launch_ok, l.d_cells = off(l.d_cells, 4));
    REJECT(group_launch_ok, l.d_slots = nullptr);
    REJECT(group_launch_ok, l.d_side_rec = nullptr);
    REJECT(group_launch_ok, l.d_running = nullptr);
    REJECT(group_launch_ok, l.d_side_cell = nullptr);
    REJECT(group_launch_ok, l.ncols = 0u; d.text = 1u; l.d_side_cell = nullptr);               /* a key cell is a cell */
    ACCEPT(group_launch_ok, l.ncols = 0u; l.d_side_cell = nullptr; l.d_cells = nullptr);       /* a group without cells */
    REJECT(group_launch_ok, l.d_rec = nullptr);
    REJECT(group_launch_ok, l.d_cells = nullptr);
    ACCEPT(group_launch_ok, l.group_cap = 0u; l.d_rec = nullptr; l.d_cells = nullptr);
}

static void check_project()
{
    ProjectLaunch l0;
    l0.d_cols = at<const void>(0x300208);
    l0.ncols = 8;
    l0.row_bytes = 64;
    l0.d_blocks = at<uint4>(0x400000);
    l0.d_side_rec = at<void>(0x500008);
    l0.d_side_rows = at<void>(0x580008);
    l0.d_running = at<uint64_t>(0x600008);
    l0.d_rec = at<void>(0x700008);
    l0.rec_cap = 100;
    l0.d_rows = at<void>(0x800008);
    l0.row_cap = 100;
    check_common(project_launch_ok, l0);
    const ScanChunk c0 = good_chunk();
    const ScanDesc d0 = good_desc();
    ACCEPT(project_launch_ok, l.ncols = 1u; l.row_bytes = 8u);
    REJECT(project_launch_ok, l.ncols = 0u);
    REJECT(project_launch_ok, l.ncols = 9u);
    REJECT(project_launch_ok, l.row_bytes = 0u);
    REJECT(project_launch_ok, l.row_bytes = 4u);
    REJECT(project_launch_ok, l.row_bytes = 12u);
    REJECT(project_launch_ok, l.row_bytes = 72u);
    REJECT(project_launch_ok, l.d_cols = off(l.d_cols, 4));
    REJECT(project_launch_ok, l.d_side_rec = off(l.d_side_rec, 4));
    REJECT(project_launch_ok, l.d_side_rows = off(l.d_side_rows, 4));
    REJECT(project_launch_ok, l.d_running = off(l.d_running, 4));
    REJECT(project_launch_ok, l.d_rec = off(l.d_rec, 4));
    REJECT(project_launch_ok, l.d_rows = off(l.d_rows, 4));
    REJECT(project_launch_ok, l.d_cols = nullptr);
    REJECT(project_launch_ok, l.d_side_rec = nullptr);
    REJECT(project_launch_ok, l.d_side_rows = nullptr);
    REJECT(project_launch_ok, l.d_running = nullptr);
    REJECT(project_launch_ok, l.d_rec = nullptr);
    ACCEPT(project_launch_ok, l.d_rec = nullptr; l.rec_cap = 0u);
    REJECT(project_launch_ok, l.d_rows = nullptr);
    ACCEPT(project_launch_ok, l.d_rows = nullptr; l.row_cap = 0u);
}

/* ORDER BY int4 DESC NULLS FIRST, float4; the row: columns of width 1, 4, 8 at offsets 0, 4, 8 */
static const cryo_agg_col kTopnTable[CRYO_ORDER_MAX_BY + CRYO_PROJECT_MAX_COLS] = {
    {1, CRYO_KEY_INT4, CRYO_ORDER_DESC | CRYO_ORDER_NULLS_FIRST, 0}, {2, CRYO_KEY_FLOAT4, 0, 0}, {3, 1, 0, 0}, {1, 4, 4, 0}, {4, 8, 8, 0},
};

static void check_topn()
{
    TopnLaunch l0;
    l0.d_slots = at<const void>(0x300208);
    l0.h_slots = kTopnTable;
    l0.nby = 2;
    l0.ncols = 3;
    l0.row_bytes = 16;
    l0.limit = 1;
    l0.d_blocks = at<uint4>(0x400000);
    l0.d_side_rec = at<void>(0x500008);
    l0.d_side_rows = at<void>(0x580008);
    l0.d_side_ord = at<void>(0x5c0004);
    l0.d_running = at<uint64_t>(0x600008);
    l0.d_rec = at<void>(0x700008);
    l0.d_rows = at<void>(0x800008);
    l0.row_cap = 100;
    check_common(topn_launch_ok, l0);
    const ScanChunk c0 = good_chunk();
    const ScanDesc d0 = good_desc();
    ACCEPT(topn_launch_ok, l.nby = 1u; l.ncols = 8u; l.row_bytes = 64u);
    REJECT(topn_launch_ok, l.nby = 0u);
    REJECT(topn_launch_ok, l.nby = 3u);
    REJECT(topn_launch_ok, l.limit = 0u);
    REJECT(topn_launch_ok, l.ncols = 0u);
    REJECT(topn_launch_ok, l.ncols = 9u);
    REJECT(topn_launch_ok, l.row_bytes = 0u);
    REJECT(topn_launch_ok, l.row_bytes = 4u);
    REJECT(topn_launch_ok, l.row_bytes = 12u);
    REJECT(topn_launch_ok, l.row_bytes = 72u);
    REJECT(topn_launch_ok, l.d_slots = off(l.d_slots, 4));
    REJECT(topn_launch_ok, l.d_side_rec = off(l.d_side_rec, 4));
    REJECT(topn_launch_ok, l.d_side_rows = off(l.d_side_rows, 4));
    REJECT(topn_launch_ok, l.d_side_ord = off(l.d_side_ord, 2));
    REJECT(topn_launch_ok, l.d_running = off(l.d_running, 4));
    REJECT(topn_launch_ok, l.d_rec = off(l.d_rec, 4));
    REJECT(topn_launch_ok, l.d_rows = off(l.d_rows, 4));
    REJECT(topn_launch_ok, l.d_slots = nullptr);
    REJECT(topn_launch_ok, l.h_slots = nullptr);
    REJECT(topn_launch_ok, l.d_side_rec = nullptr);
    REJECT(topn_launch_ok, l.d_side_rows = nullptr);
    REJECT(topn_launch_ok, l.d_side_ord = nullptr);
    REJECT(topn_launch_ok, l.d_running = nullptr);
    REJECT(topn_launch_ok, l.d_rec = nullptr);
    REJECT(topn_launch_ok, l.d_rows = nullptr);
    ACCEPT(topn_launch_ok, l.d_rec = nullptr; l.d_rows = nullptr; l.row_cap = 0u);

    uint32_t ord_bits = 0;
    uint64_t row_map = 0;
    CHECK(topn_pack(l0, ord_bits, row_map) && ord_bits == 0x70719u && row_map == 0xC88400ull);
    TopnLaunch one = l0; /* the first order column and the first row column alone */
    one.nby = one.ncols = 1;
    one.row_bytes = 8;
    CHECK(topn_pack(one, ord_bits, row_map) && ord_bits == 0x10019u && row_map == 0ull);
    cryo_agg_col bad[CRYO_ORDER_MAX_BY + CRYO_PROJECT_MAX_COLS];
    TopnLaunch lb = l0;
    lb.h_slots = bad;
    memcpy(bad, kTopnTable, sizeof bad);
    CHECK(topn_pack(lb, ord_bits, row_map));
    bad[3].type = 3; /* a width of 3 */
    CHECK(!topn_pack(lb, ord_bits, row_map));
    memcpy(bad, kTopnTable, sizeof bad);
    bad[3].rsv = 2; /* a 4-byte column at offset 2 */
    CHECK(!topn_pack(lb, ord_bits, row_map));
    memcpy(bad, kTopnTable, sizeof bad);
    bad[4].rsv = 16; /* an 8-byte column at offset 16 of a 16-byte row */
    CHECK(!topn_pack(lb, ord_bits, row_map));
    bad[4].rsv = 8;
    lb.row_bytes = 8; /* the same column, in place, beyond a row of 8 bytes */
    CHECK(!topn_pack(lb, ord_bits, row_map));
}

int main()
{
    check_routes();
    check_packing_and_grid();
    check_filter();
    check_agg();
    check_group();
    check_project();
    check_topn();
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("scan launch check ok\n");
    return 0;
}
