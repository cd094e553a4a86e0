// The traceback driver's layout and split (rawalign_amd/csrc/rawdtw_tb_layout.h) as a plain C++ program: the header needs no HIP.
//   no argument   over cnt jobs x acc path elements, steps form and text form, with and without the extra word, records of 0 and of an
//                 odd size: every region of a slot's device path block, landing zone and text block starts on a 256-byte boundary,
//                 lies inside the slot and overlaps no other, in slot 0 and in slot 1 of a block of block_bytes(need); slot 1 starts at
//                 half the block; a region is at least what is written to it; the totals equal what traceback_core (dev_need,
//                 host_need, text_need), band_traceback and semi_traceback (their `need` sums) computed by hand, restated here.
//                 Prints "ok <cases>"; the first failure otherwise.
//   "split"       reads a budget and then one job's direction bytes a number from standard input, prints "begin cnt" a sub-batch.
#include <cstring>

#include "layout_check.h"
#include "rawdtw_tb_layout.h"

using namespace rawdtw;

// the regions of one slot at its place in a two-slot block
static bool slots_ok(const char *block, std::vector<Named> rs, size_t need)
{
    const size_t bytes = tb::block_bytes(need);
    if (bytes < 2 * need || bytes % 512) { printf("FAIL %s: a block of %zu bytes for two slots of %zu\n", block, bytes, need); return false; }
    if (tb::slot_at(bytes, 0) != 0 || tb::slot_at(bytes, 1) != bytes / 2) { printf("FAIL %s: slot 1 does not start at half the block\n", block); return false; }
    if (!regions_ok(block, rs, need, 256)) return false;
    for (Named &x : rs) x.r.at += tb::slot_at(bytes, 1);
    if (tb::slot_at(bytes, 1) < need) { printf("FAIL %s: slot 1 starts inside slot 0\n", block); return false; }
    return regions_ok(block, rs, bytes, 256);
}

static int sweep()
{
    const uint64_t cnts[6] = {0, 1, 63, 64, 65, 1000};
    const uint64_t accs[6] = {0, 1, 255, 256, 257, (1ull << 32) + 5};
    const size_t recs[2] = {0, 12345};
    unsigned long long cases = 0;
    for (uint64_t cnt : cnts)
        for (uint64_t acc : accs)
            for (int text = 0; text < 2; text++)
                for (int extra = 0; extra < 2; extra++)
                    for (size_t rec : recs) {
                        cases++;
                        const tb::Paths P = tb::paths(cnt, acc, extra, rec);
                        const std::vector<Named> dev = {{"recs", P.recs, rec, rec != 0},    {"poff", P.poff, cnt * 8, true}, {"plen", P.plen, cnt * 4, true},
                                                        {"extra", P.extra, cnt * 4, !!extra}, {"ti", P.ti, acc * 4, true},     {"tj", P.tj, acc * 4, true},
                                                        {"pd", P.pd, acc * 4, true},          {"mv", P.mv, acc, true}};
                        if (!slots_ok("paths", dev, P.need)) return 1;
                        // traceback_core's dev_need; band_traceback's and semi_traceback's `need` less their records
                        const size_t dev_need = al256(cnt * 8) + al256(cnt * 4) + 3 * al256(acc * 4) + al256(acc);
                        if (P.need != al256(rec) + dev_need + (extra ? al256(cnt * 4) : 0)) { printf("FAIL paths need %zu\n", P.need); return 1; }
                        const tb::Landing H = tb::landing(cnt, acc, extra, text);
                        const std::vector<Named> pin = {{"pd", H.pd, acc * 4, !text},        {"mv", H.mv, acc, !text},           {"cost", H.cost, cnt * 4, true},
                                                        {"plen", H.plen, cnt * 4, true},     {"extra", H.extra, cnt * 4, !!extra}, {"toff", H.toff, (cnt + 1) * 8, !!text}};
                        if (!slots_ok("landing", pin, H.need)) return 1;
                        // traceback_core's host_need (it had no extra word; the other two landed in pageable vectors)
                        const size_t hacc = text ? 0 : acc;
                        const size_t host_need = al256(hacc * 4) + al256(hacc) + 2 * al256(cnt * 4) + (text ? al256((cnt + 1) * 8) : 0);
                        if (H.need != host_need + (extra ? al256(cnt * 4) : 0)) { printf("FAIL landing need %zu\n", H.need); return 1; }
                        // the places traceback_core computed by hand in finish() and at the download
                        if (H.pd.at != 0 || H.mv.at != al256(hacc * 4) || H.cost.at != al256(hacc * 4) + al256(hacc) || H.plen.at != H.cost.at + al256(cnt * 4) ||
                            (text && H.toff.at != H.cost.at + 2 * al256(cnt * 4) + (extra ? al256(cnt * 4) : 0))) {
                            printf("FAIL a landing region is not where traceback_core had it\n");
                            return 1;
                        }
                        const uint64_t bound = acc; // (any number serves as a text bound)
                        const tb::Text X = tb::text(cnt, bound);
                        const std::vector<Named> txt = {{"rec", X.rec, cnt * 32, true}, {"tot", X.tot, cnt * 8, true}, {"toff", X.toff, (cnt + 1) * 8, true}, {"text", X.text, bound + 16, true}};
                        if (!slots_ok("text", txt, X.need)) return 1;
                        const size_t text_need = al256(cnt * 32) + al256(cnt * 8) + al256((cnt + 1) * 8) + al256(bound + 16);
                        if (X.need != text_need) { printf("FAIL text need %zu, traceback_core had %zu\n", X.need, text_need); return 1; }
                        // the paths' own records: sizeof(DevJob) = 32 and sizeof(FullAux) = 16 in the library; an odd pair here as well
                        for (int odd = 0; odd < 2; odd++) {
                            const size_t jb = odd ? 33 : 32, ab = odd ? 7 : 16;
                            const uint64_t bnd = acc < (1u << 20) ? acc : 77;
                            const tb::Recs B = tb::recs(cnt, jb, ab, false, false, 0), S = tb::recs(cnt, jb, ab, true, false, bnd), Sp = tb::recs(cnt, jb, ab, true, true, bnd);
                            const std::vector<Named> rb = {{"jobs", B.jobs, cnt * jb, true}, {"aux", B.aux, cnt * ab, true}, {"cost", B.cost, cnt * 4, true},
                                                           {"endj", B.endj, 0, false},       {"j0", B.j0, 0, false},         {"bnd", B.bnd, 0, false}};
                            const std::vector<Named> rs = {{"jobs", Sp.jobs, cnt * jb, true},  {"aux", Sp.aux, cnt * ab, true}, {"cost", Sp.cost, cnt * 4, true},
                                                           {"endj", Sp.endj, cnt * 4, true},   {"j0", Sp.j0, cnt * 4, true},    {"bnd", Sp.bnd, bnd * 4, bnd != 0}};
                            if (!regions_ok("banded records", rb, B.need, 256) || !regions_ok("semiglobal records", rs, Sp.need, 256)) return 1;
                            // band_traceback's need: records, 2 words (cost, plen), offsets, paths; semi_traceback's: 4 words (cost, end_j, plen, j0) and
                            // the boundary rows; semi_batch's: 2 or 3 words and the boundary rows
                            const size_t band_need = al256(cnt * jb) + al256(cnt * ab) + 2 * al256(cnt * 4) + al256(cnt * 8) + 3 * al256(acc * 4) + al256(acc);
                            const size_t semi_need = al256(cnt * jb) + al256(cnt * ab) + 4 * al256(cnt * 4) + al256(cnt * 8) + al256(bnd * 4) + 3 * al256(acc * 4) + al256(acc);
                            if (tb::paths(cnt, acc, false, B.need).need != band_need) { printf("FAIL the banded slot is not band_traceback's need\n"); return 1; }
                            if (tb::paths(cnt, acc, true, S.need).need != semi_need) { printf("FAIL the semiglobal slot is not semi_traceback's need\n"); return 1; }
                            if (S.need != al256(cnt * jb) + al256(cnt * ab) + 2 * al256(cnt * 4) + al256(bnd * 4) || Sp.need != S.need + al256(cnt * 4)) {
                                printf("FAIL the cost or span form's block is not semi_batch's need\n");
                                return 1;
                            }
                        }
                    }
    printf("ok %llu\n", cases);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return sweep();
    if (strcmp(argv[1], "split")) return 2;
    unsigned long long budget = 0, b = 0;
    if (scanf("%llu", &budget) != 1) return 2;
    std::vector<uint64_t> bytes;
    while (scanf("%llu", &b) == 1) bytes.push_back(b);
    for (const tb::Cut &c : tb::split(bytes.data(), bytes.size(), budget)) printf("%llu %llu\n", (unsigned long long)c.begin, (unsigned long long)c.cnt);
    return 0;
}
