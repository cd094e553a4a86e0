// rawdtw_chain_append.h -- the offsets of rawdtw_chain_round_append ("chain_decline_reads"; rawdtw_chain.hip), as pure functions of the host:
// the chains the host made for a round's declined reads go behind the device's own chains, and each declined read gets a pseudo-read at the
// end of the batch's read list.
//
//   the round as _end left it     n_reads reads, chain_off[n_reads + 1] (a declined read's stretch is empty), nc0 chains, na0 anchors
//   what the caller appends       n_decl reads' chains, app_chain_off[n_decl + 1] and app_anchor_off[nca + 1], both from 0
//   the batch after the append    n_reads + n_decl reads: pseudo-read n_reads + j is the j-th declined read (ascending read order) and owns
//                                 chains [nc0 + app_chain_off[j], nc0 + app_chain_off[j + 1]); chain nc0 + c owns anchors
//                                 [na0 + app_anchor_off[c], na0 + app_anchor_off[c + 1])
// Every read's chains are contiguous and in evaluation order, which is all rawdtw_batch_submit_device asks.
// Tested alone, plain and under the sanitizers, by tests/abi/chain_append.cpp.
#pragma once
#include <cstdint>

namespace rawdtw {
namespace chain_append {

enum : int { kOk = 0, kBadOffsets = 1, kNoRoom = 2 };

// the batch's read that carries the j-th declined read's chains
inline uint64_t pseudo_read(const uint64_t n_reads, const uint64_t j) { return n_reads + j; }

// kBadOffsets: an offset array that does not start at 0 or descends, or a round whose chain_off does not end at nc0.
// kNoRoom: more chains than chains_room or more anchors than anchors_room after the append -- nothing was written.
// kOk: chain_off_ext[n_reads + n_decl + 1] is the batch's, and anchor_off_ext[nc0 + nca + 1] the round's anchor_off[0 .. nc0] (which ends at
// na0) continued behind the device's chains.  anchor_off_ext may be anchor_off itself, where that array has the room.
inline int extend_offsets(const uint64_t n_reads, const uint64_t *chain_off, const uint64_t *anchor_off, const uint64_t nc0, const uint64_t na0,
                          const uint64_t n_decl, const uint64_t *app_chain_off, const uint64_t *app_anchor_off, const uint64_t chains_room,
                          const uint64_t anchors_room, uint64_t *chain_off_ext, uint64_t *anchor_off_ext)
{
    if (chain_off[n_reads] != nc0 || anchor_off[nc0] != na0 || app_chain_off[0] != 0 || app_anchor_off[0] != 0) return kBadOffsets;
    for (uint64_t j = 0; j < n_decl; j++) if (app_chain_off[j + 1] < app_chain_off[j]) return kBadOffsets;
    const uint64_t nca = app_chain_off[n_decl];
    for (uint64_t c = 0; c < nca; c++) if (app_anchor_off[c + 1] < app_anchor_off[c]) return kBadOffsets;
    const uint64_t naa = app_anchor_off[nca];
    if (nca > chains_room || nc0 > chains_room - nca || naa > anchors_room || na0 > anchors_room - naa) return kNoRoom;
    for (uint64_t r = 0; r <= n_reads; r++) chain_off_ext[r] = chain_off[r];
    for (uint64_t j = 0; j <= n_decl; j++) chain_off_ext[pseudo_read(n_reads, j)] = nc0 + app_chain_off[j];
    for (uint64_t c = 0; c <= nc0; c++) anchor_off_ext[c] = anchor_off[c];
    for (uint64_t c = 0; c <= nca; c++) anchor_off_ext[nc0 + c] = na0 + app_anchor_off[c];
    return kOk;
}

} // namespace chain_append
} // namespace rawdtw
