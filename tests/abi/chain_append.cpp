// chain_append.cpp -- rawalign_amd/csrc/rawdtw_chain_append.h alone, with its own main: the offsets rawdtw_chain_round_append computes when the
// host's chains of a round's declined reads go behind the device's ("chain_decline_reads").  Every array is allocated at exactly the size
// the header documents, so that a sanitizer build sees any access past it.  Prints "ok <cases>".
#include "rawdtw_chain_append.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace rawdtw::chain_append;

static int cases = 0;
#define CHECK(c) do { if (!(c)) { std::printf("failed: %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

// a round of n_reads reads of which every `step`-th is declined, `per` chains a read of `len` anchors each
static void run_case(const uint64_t n_reads, const uint64_t step, const uint64_t per, const uint64_t len, const uint64_t slack)
{
    std::vector<uint64_t> chain_off(n_reads + 1, 0), declined;
    for (uint64_t r = 0; r < n_reads; r++) {
        const bool d = step && r % step == step - 1;
        if (d) declined.push_back(r);
        chain_off[r + 1] = chain_off[r] + (d ? 0 : per);
    }
    const uint64_t nc0 = chain_off[n_reads], na0 = nc0 * len, nd = declined.size();
    std::vector<uint64_t> app_coff(nd + 1, 0);
    for (uint64_t j = 0; j < nd; j++) app_coff[j + 1] = app_coff[j] + (j % 3 == 1 ? 0 : per + j % 2); // (a declined read without chains among them)
    const uint64_t nca = app_coff[nd];
    std::vector<uint64_t> app_aoff(nca + 1, 0);
    for (uint64_t c = 0; c < nca; c++) app_aoff[c + 1] = app_aoff[c] + len + c % 3;
    const uint64_t naa = app_aoff[nca];
    const uint64_t chains_room = nc0 + nca + slack, anchors_room = na0 + naa + slack;
    std::vector<uint64_t> anchor_off(chains_room + 1, 0), ext(n_reads + nd + 1, ~0ull);
    for (uint64_t c = 0; c <= nc0; c++) anchor_off[c] = c * len;
    CHECK(extend_offsets(n_reads, chain_off.data(), anchor_off.data(), nc0, na0, nd, app_coff.data(), app_aoff.data(), chains_room, anchors_room, ext.data(), anchor_off.data()) == kOk);
    // the round's reads as they were, the declined ones empty; every pseudo-read its read's chains, contiguous, behind the device's
    for (uint64_t r = 0; r <= n_reads; r++) CHECK(ext[r] == chain_off[r]);
    for (uint64_t j = 0; j < nd; j++) {
        CHECK(chain_off[declined[j]] == chain_off[declined[j] + 1]);
        CHECK(ext[pseudo_read(n_reads, j)] == nc0 + app_coff[j] && ext[pseudo_read(n_reads, j) + 1] == nc0 + app_coff[j + 1]);
    }
    for (uint64_t p = 0; p < n_reads + nd; p++) CHECK(ext[p] <= ext[p + 1]);
    CHECK(ext[n_reads + nd] == nc0 + nca);
    for (uint64_t c = 0; c < nc0; c++) CHECK(anchor_off[c + 1] - anchor_off[c] == len);
    for (uint64_t c = 0; c < nca; c++) CHECK(anchor_off[nc0 + c + 1] - anchor_off[nc0 + c] == app_aoff[c + 1] - app_aoff[c]);
    CHECK(anchor_off[nc0 + nca] == na0 + naa);
    // ... and the same into an array of its own, of exactly nc0 + nca + 1 entries, from the round's of nc0 + 1
    std::vector<uint64_t> own(anchor_off.begin(), anchor_off.begin() + nc0 + 1), sep(nc0 + nca + 1, ~0ull), ext1(n_reads + nd + 1, ~0ull);
    CHECK(extend_offsets(n_reads, chain_off.data(), own.data(), nc0, na0, nd, app_coff.data(), app_aoff.data(), chains_room, anchors_room, ext1.data(), sep.data()) == kOk);
    CHECK(ext1 == ext);
    for (uint64_t c = 0; c <= nc0 + nca; c++) CHECK(sep[c] == anchor_off[c]);
    cases++;
    // no room for the last chain, or for the last anchor: refused, nothing written
    if (nca) {
        std::vector<uint64_t> ao2(nc0 + nca, 7), ext2(n_reads + nd + 1, 7);
        CHECK(extend_offsets(n_reads, chain_off.data(), anchor_off.data(), nc0, na0, nd, app_coff.data(), app_aoff.data(), nc0 + nca - 1, anchors_room, ext2.data(), ao2.data()) == kNoRoom);
        CHECK(extend_offsets(n_reads, chain_off.data(), anchor_off.data(), nc0, na0, nd, app_coff.data(), app_aoff.data(), chains_room, na0 + naa - 1, ext2.data(), ao2.data()) == kNoRoom);
        for (uint64_t x : ao2) CHECK(x == 7);
        for (uint64_t x : ext2) CHECK(x == 7);
        cases++;
    }
}

int main()
{
    for (uint64_t n_reads : {1ull, 2ull, 3ull, 10ull, 64ull, 601ull})
        for (uint64_t step : {0ull, 1ull, 2ull, 3ull, 7ull})
            for (uint64_t per : {0ull, 1ull, 5ull})
                for (uint64_t len : {1ull, 2ull, 9ull})
                    run_case(n_reads, step, per, len, (n_reads + step) % 2);
    // offsets that do not start at 0, descend, or a round whose chain_off does not end at nc0
    {
        const uint64_t chain_off[3] = {0, 2, 2}, good_c[2] = {0, 1}, good_a[2] = {0, 3};
        uint64_t ext[4] = {9, 9, 9, 9}, ao[4] = {0, 2, 4, 9};
        const uint64_t bad_c0[2] = {1, 1}, bad_c1[2] = {0, 1}, bad_a0[2] = {1, 3}, bad_a1[2] = {0, 3};
        CHECK(extend_offsets(2, chain_off, ao, 2, 4, 1, bad_c0, good_a, 8, 8, ext, ao) == kBadOffsets);
        CHECK(extend_offsets(2, chain_off, ao, 2, 4, 1, good_c, bad_a0, 8, 8, ext, ao) == kBadOffsets);
        CHECK(extend_offsets(2, chain_off, ao, 3, 4, 1, good_c, good_a, 8, 8, ext, ao) == kBadOffsets);
        const uint64_t desc_c[3] = {0, 2, 1}, desc_a[3] = {0, 3, 2};
        uint64_t ext3[5] = {9, 9, 9, 9, 9};
        CHECK(extend_offsets(2, chain_off, ao, 2, 4, 2, desc_c, desc_a, 8, 8, ext3, ao) == kBadOffsets);
        const uint64_t two_c[2] = {0, 2};
        CHECK(extend_offsets(2, chain_off, ao, 2, 4, 1, two_c, desc_a, 8, 8, ext, ao) == kBadOffsets);
        CHECK(ext[0] == 9 && ao[3] == 9);
        CHECK(extend_offsets(2, chain_off, ao, 2, 4, 1, bad_c1, bad_a1, 3, 7, ext, ao) == kOk && ext[2] == 2 && ext[3] == 3 && ao[2] == 4 && ao[3] == 7);
        cases++;
    }
    std::printf("ok %d\n", cases);
    return 0;
}
