// The layout of the semiglobal traceback in windows (rawalign_amd/csrc/rawdtw_semi_window.h) as a plain C++ program: the header needs
// no HIP.
//   no argument   over n x m x C: a job is windowed iff C != 0 and m > C; a windowed job's two regions (one window's directions, its
//                 checkpoints) start on 256-byte boundaries, lie inside the job's stretch and do not overlap; every checkpoint column
//                 k C - 1 < m has its n floats inside the checkpoints, no two of them overlap, and there is none for a column >= m;
//                 lo(j) <= j < lo(j) + C, lo(j) a multiple of C, and a window is never wider than width(m, C); the setter's values.
//                 Prints "ok <cases>"; the first failure otherwise.
//   "jobs"        reads C and then "n m" a job from standard input; prints "windowed dir_bytes ckpt_off ckpt_bytes job_bytes offset" a
//                 job, offset the job's place in a workspace laid out in job order (64-bit).
//   "split"       reads a budget, C and then "n m" a job; prints "begin cnt" a sub-batch of rawdtw_tb_layout.h's split over what the
//                 split counts for each job (a job that is not windowed: semi_dir_bytes + 256, restated here).
#include <cstdio>
#include <cstring>
#include <vector>

#include "rawdtw_semi_window.h"
#include "rawdtw_tb_layout.h"

using namespace rawdtw;
namespace sw = rawdtw::semi_window;

static uint32_t rpl_of(uint32_t n) { return n <= 64 ? 1 : n <= 128 ? 2 : n <= 256 ? 4 : 8; }

// semi_dir_bytes (rawdtw_semiglobal.h) restated: the n x m form
static uint64_t full_dir_bytes(uint32_t n, uint32_t m)
{
    const uint64_t rpl = rpl_of(n), strips = (n + 64 * rpl - 1) / (64 * rpl), spb = rpl == 8 ? 8 : 16;
    return strips * (((uint64_t)m + 63 + spb - 1) / spb) * 64 * 16;
}

static uint64_t split_bytes(uint32_t n, uint32_t m, uint32_t C)
{
    return sw::windowed(m, C) ? sw::job_bytes(n, m, C, rpl_of(n)) : full_dir_bytes(n, m) + 256;
}

static int sweep()
{
    const uint32_t ns[] = {1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1025, 1537, 1u << 20};
    const uint32_t ms[] = {1, 63, 64, 65, 127, 128, 129, 200, 1000, 4096, 29903, (1u << 21) + 5};
    const uint32_t Cs[] = {0, 64, 128, 512, 1024, 4096, 1u << 20};
    unsigned long long cases = 0;
    for (uint32_t n : ns)
        for (uint32_t m : ms)
            for (uint32_t C : Cs) {
                cases++;
                const bool w = sw::windowed(m, C);
                if (w != (C != 0 && m > C)) { printf("FAIL windowed(%u, %u)\n", m, C); return 1; }
                if (!w) continue;
                const uint32_t rpl = rpl_of(n);
                const uint64_t db = sw::dir_bytes(n, m, C, rpl), co = sw::ckpt_off(n, m, C, rpl), cb = sw::ckpt_bytes(n, m, C), jb = sw::job_bytes(n, m, C, rpl);
                if (db != full_dir_bytes(n, C) || sw::width(m, C) != C) { printf("FAIL dir_bytes(%u, %u, %u) is not the n x C form's\n", n, m, C); return 1; }
                if (co % 256 || cb % 256 || co < db || jb != co + cb) { printf("FAIL regions of (%u, %u, %u)\n", n, m, C); return 1; }
                // checkpoints: k = 1 .. m / C, column k C - 1 < m, the next one would lie at or past m
                const uint64_t K = sw::checkpoints(m, C);
                if (K == 0 || K * C - 1 >= m || (K + 1) * (uint64_t)C - 1 < m) { printf("FAIL checkpoints(%u, %u) = %llu\n", m, C, (unsigned long long)K); return 1; }
                if (sw::ckpt_floats(n, m, C) != K * n || cb < K * n * 4) { printf("FAIL checkpoint floats of (%u, %u, %u)\n", n, m, C); return 1; }
                uint64_t before = 0;
                for (uint64_t k = 1; k <= K; k += (K > 64 ? K / 7 : 1)) {
                    const uint64_t at = sw::ckpt_at(n, C, (uint32_t)(k * C - 1));
                    if (at != (k - 1) * n || (at + n) * 4 > cb || (k > 1 && at < before)) { printf("FAIL ckpt_at(%u, %u, column %llu)\n", n, C, (unsigned long long)(k * C - 1)); return 1; }
                    before = at + n;
                }
                const uint32_t js[] = {0, 1, C - 1, C, C + 1, m / 2, m - 1};
                for (uint32_t j : js) {
                    if (j >= m) continue;
                    const uint32_t lo = sw::lo(j, C);
                    if (lo % C || lo > j || j - lo >= C || j - lo + 1 > sw::width(m, C)) { printf("FAIL lo(%u, %u)\n", j, C); return 1; }
                    if (lo && (sw::ckpt_at(n, C, lo - 1) + n) * 4 > cb) { printf("FAIL the checkpoint in front of lo(%u, %u)\n", j, C); return 1; }
                }
            }
    const uint64_t good[] = {0, 64, 128, 4096, 1u << 20}, bad[] = {1, 63, 65, 100, (1u << 20) + 64, 1u << 21, 0xffffffc0ull};
    for (uint64_t c : good) if (!sw::valid_columns(c)) { printf("FAIL valid_columns(%llu)\n", (unsigned long long)c); return 1; }
    for (uint64_t c : bad) if (sw::valid_columns(c)) { printf("FAIL valid_columns(%llu)\n", (unsigned long long)c); return 1; }
    printf("ok %llu\n", cases);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return sweep();
    unsigned long long budget = 0, C = 0, n = 0, m = 0;
    if (!strcmp(argv[1], "jobs")) {
        if (scanf("%llu", &C) != 1) return 2;
        uint64_t off = 0;
        while (scanf("%llu %llu", &n, &m) == 2) {
            const bool w = sw::windowed((uint32_t)m, (uint32_t)C);
            const uint32_t rpl = rpl_of((uint32_t)n);
            const uint64_t db = w ? sw::dir_bytes(n, m, C, rpl) : full_dir_bytes(n, m), co = w ? sw::ckpt_off(n, m, C, rpl) : 0, cb = w ? sw::ckpt_bytes(n, m, C) : 0;
            const uint64_t jb = w ? sw::job_bytes(n, m, C, rpl) : sw::al256(db);
            printf("%d %llu %llu %llu %llu %llu\n", (int)w, (unsigned long long)db, (unsigned long long)co, (unsigned long long)cb, (unsigned long long)jb, (unsigned long long)off);
            off += jb;
        }
        return 0;
    }
    if (strcmp(argv[1], "split")) return 2;
    if (scanf("%llu %llu", &budget, &C) != 2) return 2;
    std::vector<uint64_t> bytes;
    while (scanf("%llu %llu", &n, &m) == 2) bytes.push_back(split_bytes((uint32_t)n, (uint32_t)m, (uint32_t)C));
    for (const tb::Cut &c : tb::split(bytes.data(), bytes.size(), budget)) printf("%llu %llu\n", (unsigned long long)c.begin, (unsigned long long)c.cnt);
    return 0;
}
