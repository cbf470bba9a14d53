// Host check of the LDS plan of k_env_rollout_act_free (ms_layout.h free_lds), run by tests/test_lds_plan.py.
//
// The kernel's wave w steps its replicas in the slot [w * free_slot, (w + 1) * free_slot) of the workgroup's
// dynamic LDS and, at the start of a round, may twist an MT19937 block in the first 4 * kMtN bytes of that slot
// (env_round -> mt_refill_groups) while the other waves' slots and the act area (pdig, list, accx, pace) hold
// live data. For every shape the config check accepts (capi.cpp check_config: N <= 64, C <= 64, L <= 32,
// N * L <= MS_MAX_OFFERS, new jobs in [0, L]) that passes free_rollout_shape_ok this program checks
//   - the act areas are ordered, aligned and do not overlap, and start at or after the slots' end;
//   - 2 * (total + 256) <= 160 KiB exactly when free_rollout_lds_ok says so;
//   - where the shape is supported: every wave's twist range lies below pdig and, for every wave but the
//     last, inside its own slot (past the last slot only padding lies below pdig).
// Output: one "FAIL N C L J: what" line per violated check, "count <shape-ok> <supported>" (new jobs = 1) and
// "lds N C L pdig list accx pace total" for 8 x 8 x 3 and 1 x 1 x 16. Exit status 1 if anything failed.
#include <cstdio>

#include "../marl-scheduling_amd/csrc/ms_layout.h"

using namespace ms;

static int n_fail = 0;

static void fail(const Geom& g, int J, const char* what, long a, long b) {
    printf("FAIL %d %d %d %d: %s (%ld vs %ld)\n", g.N, g.C, g.L, J, what, a, b);
    n_fail++;
}

static void check(const Geom& g, int J) {
    const FreeLds f = free_lds(g);
    const long slot = free_slot(g), twist = 4 * kMtN;
    if (slot != (long)kFreeEPW * g.s_total) fail(g, J, "slot is not kFreeEPW * s_total", slot, (long)kFreeEPW * g.s_total);
    if (f.pdig < g.N * slot) fail(g, J, "pdig inside the env slots", f.pdig, g.N * slot);
    if (f.pdig % 16) fail(g, J, "pdig not 16-byte aligned", f.pdig, 16);
    if (f.list < f.pdig + 4 * 256 * 2) fail(g, J, "list overlaps pdig", f.list, f.pdig + 4 * 256 * 2);
    if (f.accx < f.list + g.N * kFreeListCap * 6) fail(g, J, "accx overlaps list", f.accx, f.list + g.N * kFreeListCap * 6);
    if (f.pace < f.accx + kFreeEPW * g.N * g.N * g.C) fail(g, J, "pace overlaps accx", f.pace, f.accx + kFreeEPW * g.N * g.N * g.C);
    if (f.total < f.pace + 4 * 8) fail(g, J, "total cuts pace", f.total, f.pace + 4 * 8);
    if ((f.list | f.accx | f.pace | f.total) & 3) fail(g, J, "act area not dword aligned", f.list | f.accx | f.pace | f.total, 4);
    const bool fits = 2 * ((long)f.total + 256) <= 160 * 1024;
    const bool ok = free_rollout_lds_ok(g);
    if (fits != ok) fail(g, J, "LDS budget and free_rollout_lds_ok disagree", fits, ok);
    if (!ok) return;
    for (int w = 0; w < g.N; w++) {
        const long lo = w * slot, hi = lo + twist;
        if (hi > f.pdig) fail(g, J, "MT twist of a wave reaches pdig", hi, f.pdig);
        if (w + 1 < g.N && hi > lo + slot) fail(g, J, "MT twist of a wave reaches the next wave's slot", hi, lo + slot);
    }
}

static void print_lds(int N, int C, int L) {
    const FreeLds f = free_lds(make_geom(N, C, L, 1));
    printf("lds %d %d %d %d %d %d %d %d\n", N, C, L, f.pdig, f.list, f.accx, f.pace, f.total);
}

int main() {
    int n_shape = 0, n_supported = 0;
    for (int N = 1; N <= MS_MAX_AGENTS; N++)
        for (int C = 1; C <= MS_MAX_CORES; C++)
            for (int L = 1; L <= MS_MAX_COLLECTION && N * L <= MS_MAX_OFFERS; L++)
                for (int J = 0; J <= L; J++) {
                    const Geom g = make_geom(N, C, L, J);
                    if (!free_rollout_shape_ok(g)) continue;
                    check(g, J);
                    if (J == 1) {
                        n_shape++;
                        n_supported += free_rollout_lds_ok(g);
                    }
                }
    printf("count %d %d\n", n_shape, n_supported);
    print_lds(8, 8, 3);
    print_lds(1, 1, 16);
    return n_fail ? 1 : 0;
}
