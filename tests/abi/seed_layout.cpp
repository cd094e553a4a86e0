// The seeding workspace's layout (rawalign_amd/csrc/rawdtw_seed_layout.h) as a plain C++ program: the header needs no HIP.
// Every kind (plain, resident, detected) over n chunks x N events x w in {0, 5}:
//   device block  every region starts on a 256-byte boundary and lies inside `need`; no two non-empty regions overlap; a region is at
//                 least what its kernels index ((n + 1) * 8 for an offset array, N * 4 for a per-event word, N * 8 for val, n * 4 for a
//                 per-chunk count, 32 for tot); a region the kind does not use is empty; `need` is the sum the three begins used to write
//                 out each for itself, restated here
//   pinned block  the same: the regions disjoint, inside pin_need, where the begins and ends used to find them by hand
//                 (pin + 2, + (n + 1), + 2 (n + 1), the flag word behind the hit offsets), pin_need as it was
// Prints "ok <cases>"; the first failure otherwise.
#include "layout_check.h"
#include "rawdtw_seed_layout.h"

using namespace rawdtw::seed;

int main()
{
    const Kind kinds[3] = {Kind::plain, Kind::resident, Kind::detected};
    const uint64_t ns[6] = {0, 1, 63, 64, 65, 1000};
    unsigned long long cases = 0;
    for (int ki = 0; ki < 3; ki++)
        for (uint64_t n : ns) {
            const uint64_t Ns[6] = {0, 1, 255, 256, 257, 400 * n};
            for (uint64_t N : Ns)
                for (uint32_t w : {0u, 5u}) {
                    const Kind kind = kinds[ki];
                    const bool plain = kind == Kind::plain, resident = kind == Kind::resident, detected = kind == Kind::detected, sk = w != 0;
                    const Layout L = layout(kind, n, N, sk);
                    cases++;
                    const std::vector<Named> dev = {
                        {"off", L.off, (n + 1) * 8, true},     {"src", L.src, (n + 1) * 8, !plain},   {"ev", L.ev, N * 4, plain},
                        {"code", L.code, N * 4, true},         {"pos", L.pos, N * 4, true},           {"cnt", L.cnt, N * 4, true},
                        {"val", L.val, N * 8, true},           {"kept", L.kept, n * 4, true},         {"chits", L.chits, (n + 1) * 8, true},
                        {"hoff", L.hoff, (n + 1) * 8, true},   {"tot", L.tot, 32, true},              {"hash", L.hash, N * 4, sk},
                        {"spos", L.spos, N * 4, sk},           {"count", L.count, n * 4, sk}};
                    if (!regions_ok("device", dev, L.need, 256)) return 1;
                    // the begins' own sums, as they stood: 3 offset arrays and 4 per-event words with the events uploaded, 4 and 3 without
                    const size_t b_off = al256((n + 1) * 8), b_ev = al256(N * 4), b_val = al256(N * 8), b_cnt = al256(n * 4), b_tot = 256;
                    const size_t need = (plain ? 3 * b_off + 4 * b_ev : 4 * b_off + 3 * b_ev) + b_val + b_cnt + b_tot + (sk ? 2 * b_ev + b_cnt : 0);
                    if (L.need != need) { printf("FAIL need %zu, the begins had %zu\n", L.need, need); return 1; }
                    const std::vector<Named> pin = {
                        {"p_tot", L.p_tot, 8, true},                      {"p_over", L.p_over, 8, true},
                        {"p_off", L.p_off, (n + 1) * 8, !detected},       {"p_src", L.p_src, n * 8, resident},
                        {"p_hoff", L.p_hoff, (n + 1) * 8, !plain},        {"p_decl", L.p_decl, 8, detected}};
                    if (!regions_ok("pinned", pin, L.pin_need, 8)) return 1;
                    const size_t pin_need = plain ? (n + 3) * 8 : (3 * (n + 1) + 4) * 8;
                    if (L.pin_need != pin_need) { printf("FAIL pin_need %zu, the begins had %zu\n", L.pin_need, pin_need); return 1; }
                    // words 0 and 1 (one 16-byte copy brings both home), the offsets from word 2, the rest a row of n + 1 words apart
                    bool at = L.p_tot.at == 0 && L.p_over.at == 8 && L.p_off.at == 16;
                    if (!plain) at = at && L.p_src.at == (2 + (n + 1)) * 8 && L.p_hoff.at == (2 + 2 * (n + 1)) * 8 && L.p_decl.at == (2 + 3 * (n + 1)) * 8;
                    if (!at) { printf("FAIL a pinned region is not where the begins and ends had it\n"); return 1; }
                }
        }
    printf("ok %llu\n", cases);
    return 0;
}
