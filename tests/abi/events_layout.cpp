// The detection workspace's layout (rawalign_amd/csrc/rawdtw_events_layout.h) as a plain C++ program: the header needs no HIP.
// Every kind (float or raw, plain or resident) over n chunks x N samples:
//   device block  every region starts on a 256-byte boundary and lies inside `need`; no two non-empty regions overlap; a region is at
//                 least what its kernels index ((n + 1) * 8 for an offset array, N * 4 for a per-sample word, (N + n) * 4 for the prefix
//                 sums, whose chunk k starts at off[k] + k, n * 4 for a per-chunk count, N * 2 + 16 for the raw samples and the last
//                 window's last load, 32 for tot); a region the kind does not use is empty; `need` is the sum detect_enqueue used to
//                 write out, restated here; 28 bytes a sample (30 a raw sample) as include/rawdtw.h promises
//   pinned block  the regions disjoint, inside pin_need, aligned for their words, where detect_enqueue and the two ends used to find
//                 them by hand (word 0, word 1, pin + (arena ? 2 : 1), the places n + 1 words on, then three uint32 rows), pin_need
//                 as it was
// Prints "ok <cases>"; the first failure otherwise.
#include "layout_check.h"
#include "rawdtw_events_layout.h"

using namespace rawdtw::events;

int main()
{
    static_assert(kTotEvents == 0 && kTotSamples == 1 && kTotFlag == 2 && (kTotFlag + 1) * 8 <= 32, "tot's words");
    const uint64_t ns[6] = {0, 1, 63, 64, 65, 1000};
    unsigned long long cases = 0;
    for (int raw = 0; raw < 2; raw++)
        for (int arena = 0; arena < 2; arena++)
            for (uint64_t n : ns) {
                const uint64_t Ns[6] = {0, 1, 255, 256, 257, 4000 * n};
                for (uint64_t N : Ns) {
                    const Layout L = layout(raw, arena, n, N);
                    cases++;
                    const size_t chan = n * sizeof(rawdtw_channel_t);
                    const std::vector<Named> dev = {
                        {"off", L.off, (n + 1) * 8, true},    {"sig", L.sig, N * 4, true},          {"ps", L.ps, (N + n) * 4, true},
                        {"pss", L.pss, (N + n) * 4, true},    {"t1", L.t1, N * 4, true},            {"t2", L.t2, N * 4, true},
                        {"peaks", L.peaks, N * 4, true},      {"npk", L.npk, n * 4, true},          {"nev", L.nev, n * 4, true},
                        {"eoff", L.eoff, (n + 1) * 8, true},  {"tot", L.tot, 32, true},             {"ev", L.ev, N * 4, true},
                        {"raw", L.raw, N * 2 + 16, !!raw},    {"roff", L.roff, (n + 1) * 8, !!raw}, {"chan", L.chan, chan, !!raw},
                        {"slen", L.slen, n * 4, !!raw},       {"dst", L.dst, n * 8, !!arena},       {"room", L.room, n * 4, !!arena}};
                    if (!regions_ok("device", dev, L.need, 256)) return 1;
                    // detect_enqueue's own sum, as it stood
                    const size_t b_off = al256((n + 1) * 8), b_sig = al256(N * 4), b_ps = al256((N + n) * 4), b_t = al256(N * 4), b_cnt = al256(n * 4),
                                 b_eoff = al256((n + 1) * 8), b_tot = al256(32);
                    const size_t b_raw = raw ? al256(N * 2 + 16) : 0, b_roff = raw ? b_off : 0, b_chan = raw ? al256(chan) : 0, b_slen = raw ? b_cnt : 0;
                    const size_t b_dst = arena ? b_off : 0, b_room = arena ? b_cnt : 0;
                    const size_t need = b_off + b_sig + 2 * b_ps + 2 * b_t + b_t + 2 * b_cnt + b_eoff + b_tot + b_t + b_raw + b_roff + b_chan + b_slen + b_dst + b_room;
                    if (L.need != need) { printf("FAIL need %zu, detect_enqueue had %zu\n", L.need, need); return 1; }
                    if (L.dst.bytes != b_dst) { printf("FAIL dst has %zu bytes, detect_enqueue gave it a whole offsets row, %zu\n", L.dst.bytes, b_dst); return 1; }
                    // 28 bytes a sample (30 a raw sample) for n << N: above that only the per-chunk arrays (at most 72 bytes a chunk: four
                    // offset rows, a prefix-sum slot twice, four counts, a channel), tot's 256 bytes and the rounding of the 17 other regions
                    if (n && N == 4000 * n) {
                        const size_t samples = (raw ? 30 : 28) * N;
                        if (L.need < samples || L.need - samples > 72 * (n + 1) + 256 + 17 * 255) {
                            printf("FAIL need %zu is not %d bytes a sample (%zu) plus the per-chunk arrays and the rounding\n", L.need, raw ? 30 : 28, samples);
                            return 1;
                        }
                    }
                    const std::vector<Named> pin = {
                        {"p_tot", L.p_tot, 8, true},                   {"p_flag", L.p_flag, 8, !!arena},           {"p_off", L.p_off, (n + 1) * 8, true},
                        {"p_dst", L.p_dst, n * 8, !!arena},            {"p_room", L.p_room, n * 4, !!arena},       {"p_nev", L.p_nev, n * 4, !!arena},
                        {"p_cnt", L.p_cnt, n * 4, raw && arena}};
                    if (!regions_ok("pinned", pin, L.pin_need, 4)) return 1;
                    if (L.p_tot.at % 8 || L.p_flag.at % 8 || L.p_off.at % 8 || L.p_dst.at % 8) { printf("FAIL a pinned uint64 region is not 8-aligned\n"); return 1; }
                    const size_t pin_need = arena ? (4 * n + 4) * 8 : (n + 2) * 8;
                    if (L.pin_need != pin_need) { printf("FAIL pin_need %zu, detect_enqueue had %zu\n", L.pin_need, pin_need); return 1; }
                    // pin[0], pin[1], h_off = pin + (arena ? 2 : 1), h_dst = h_off + (n + 1), h_room = (uint32 *)(h_dst + n), h_nev = h_room + n, h_cnt = h_nev + n
                    const size_t h_off = (arena ? 2 : 1) * 8, h_dst = h_off + (n + 1) * 8, h_room = h_dst + n * 8, h_nev = h_room + n * 4, h_cnt = h_nev + n * 4;
                    bool at = L.p_tot.at == 0 && L.p_off.at == h_off;
                    if (arena) at = at && L.p_flag.at == 8 && L.p_dst.at == h_dst && L.p_room.at == h_room && L.p_nev.at == h_nev && L.p_cnt.at == h_cnt;
                    if (!at) { printf("FAIL a pinned region is not where detect_enqueue and the ends had it\n"); return 1; }
                }
            }
    printf("ok %llu\n", cases);
    return 0;
}
