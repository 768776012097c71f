/*
 * multi_share.h -- what the cryo_multi_* calls share: the deal of a call's blocks to the handles, a share's region of an
 * output buffer, and the way a share's packed per-block results go back into call order.  Plain integer code: no HIP, nothing
 * of cryo_codec, so a host-only program can include it (tests/multi_share_check.cpp does).  The comments of the cryo_multi_*
 * calls in include/cryo_codec.h are the contract this implements.
 */
#ifndef CRYO_MULTI_SHARE_H
#define CRYO_MULTI_SHARE_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace cryo {

/* ---- the deal: block i of a call of n goes to handle i mod G, so handle g holds the blocks g, g + G, ... in that order ---- */
struct RoundRobin {
    size_t n, G;
    /* the blocks of handle g */
    size_t count(size_t g) const { return g < n ? (n - g + G - 1) / G : 0; }
    /* the blocks of the handles before g */
    uint64_t before(size_t g) const
    {
        uint64_t b = 0;
        for (size_t q = 0; q < g; q++) b += count(q);
        return b;
    }
    /* the inverse: block i is entry entry_of(i) of handle handle_of(i)'s share */
    size_t handle_of(size_t i) const { return i % G; }
    size_t entry_of(size_t i) const { return i / G; }
};

/* the block indices of every handle's share, ascending; owner(i) names block i's handle (below G) */
template <class Owner>
std::vector<std::vector<size_t>> deal_shares(size_t n, size_t G, Owner owner)
{
    std::vector<std::vector<size_t>> share(G);
    for (size_t i = 0; i < n; i++) share[owner(i)].push_back(i);
    return share;
}
/* the keyed call's rule: a keyed block always goes to the same handle (its pool entry lives there), an unkeyed one
 * round-robin */
inline size_t keyed_owner(uint64_t key, size_t i, size_t G) { return (size_t)(key ? key % G : i % G); }

/* ---- a share's region of a buffer of whole_cap units: `unit` units per block, the regions in handle order, and a region that
 * reaches beyond whole_cap is cut there (none of it left: cap 0) ---- */
struct ShareRegion {
    uint64_t first = 0, cap = 0;
    ShareRegion(uint64_t whole_cap, uint64_t blocks_before, uint64_t blocks, uint64_t unit) : first(blocks_before * unit)
    {
        const uint64_t want = blocks * unit;
        cap = whole_cap > first ? (whole_cap - first < want ? whole_cap - first : want) : 0;
    }
    /* where the region starts in the buffer at `base`, whose units are `unit_size` Ts wide; null for a region with no room */
    template <class T> T *in(T *base, size_t unit_size = 1) const { return cap ? base + first * unit_size : nullptr; }
    /* the end of the last unit used when the share used `total` of them (0: none) */
    uint64_t end(uint64_t total) const { return total ? first + total : 0; }
};
/* the end of the last unit any handle used */
inline uint64_t last_end(const std::vector<uint64_t> &ends) { return ends.empty() ? 0 : *std::max_element(ends.begin(), ends.end()); }

/* ---- per-block values between call order and a share's order: `per` entries per block ---- */
template <class T> std::vector<T> gather(const std::vector<size_t> &idx, const T *in, size_t per = 1)
{
    std::vector<T> packed(idx.size() * per);
    for (size_t k = 0; k < idx.size(); k++)
        for (size_t j = 0; j < per; j++) packed[k * per + j] = in[idx[k] * per + j];
    return packed;
}
template <class T> void scatter(const std::vector<size_t> &idx, const T *packed, T *out, size_t per = 1)
{
    for (size_t k = 0; k < idx.size(); k++)
        for (size_t j = 0; j < per; j++) out[idx[k] * per + j] = packed[k * per + j];
}

} // namespace cryo

#endif
