// Host check of the packed env snapshot's layout and per-replica check (ms_snapshot.h), run by
// tests/test_snapshot_host.py, plain and under -fsanitize=address,undefined (the header needs no HIP).
//
//   - snap_layout for the shipped shapes (2x2x2, 4x4x3, 8x8x3, 16x16x3, 32x32x3) and the edges (1x1x16, 3x5x2,
//     8x11x2), several E and entry counts: every section 16-byte aligned, in order, exactly as large as its
//     content needs (restated here without the header's helpers), total = the documented formula;
//   - snap_check_replica on one valid hand-built replica of 3x5x2 (cap 4) and on one replica per violated
//     invariant: each must be refused with its own code and the index of the core / slot / agent at fault. The
//     record and the entries live in heap blocks of exactly rec_bytes and count entries, so the sanitized build
//     also shows the check reads nothing beyond them, whatever the record claims.
// Output: "FAIL ..." per violated expectation, "layout N C L E n_liab o_cfg o_recs o_mt o_off o_liab total" for
// 8x8x3 at E = 16384, "checked <layouts> <replicas>". Exit status 1 if anything failed.
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../marl-scheduling_amd/csrc/ms_snapshot.h"

using namespace ms;

static int n_fail = 0;

static unsigned long long up16(unsigned long long x) { return (x + 15) / 16 * 16; }

static void check_layout(int N, int C, int L, long long E, long long n_liab) {
    const Geom g = make_geom(N, C, L, 1);
    const SnapLayout s = snap_layout(E, g.rec_bytes, n_liab);
    auto bad = [&](const char* what, unsigned long long a, unsigned long long b) {
        printf("FAIL layout %d %d %d E %lld n %lld: %s (%llu vs %llu)\n", N, C, L, E, n_liab, what, a, b);
        n_fail++;
    };
    if (g.rec_bytes % 16) bad("rec_bytes not a multiple of 16", g.rec_bytes, 16);
    if (s.o_cfg != 64) bad("config does not follow the 64-byte header", s.o_cfg, 64);
    if (s.o_recs != up16(64 + sizeof(ms_config))) bad("o_recs", s.o_recs, up16(64 + sizeof(ms_config)));
    if (s.o_mt != s.o_recs + (unsigned long long)E * g.rec_bytes) bad("o_mt", s.o_mt, s.o_recs + E * g.rec_bytes);
    if (s.o_off != s.o_mt + (unsigned long long)E * 2496) bad("o_off", s.o_off, s.o_mt + E * 2496);
    if (s.o_liab != up16(s.o_off + 8ull * (E + 1))) bad("o_liab", s.o_liab, up16(s.o_off + 8ull * (E + 1)));
    if (s.total != up16(s.o_liab + 8ull * n_liab)) bad("total", s.total, up16(s.o_liab + 8ull * n_liab));
    const unsigned long long formula =
        up16(64 + sizeof(ms_config)) + (unsigned long long)E * (g.rec_bytes + 2496) + up16(8ull * (E + 1)) + up16(8ull * n_liab);
    if (s.total != formula) bad("total is not the documented formula", s.total, formula);
    if ((s.o_cfg | s.o_recs | s.o_mt | s.o_off | s.o_liab | s.total) & 15) bad("a section is not 16-byte aligned", 0, 0);
    // less than the raw arrays whenever the chains are not all full
    const unsigned long long cap = 128, raw = (unsigned long long)E * (g.rec_bytes + 2 * 2496 + C * cap * 8);
    if (n_liab <= E * 32 && s.total >= raw + 512) bad("snapshot not below the raw state", s.total, raw);
}

// ---- one replica of 3 x 5 x 2, two job kinds, cap 4
struct Replica {
    Params P;
    std::vector<uint8_t> rec;
    std::vector<Liab> liab;  // exactly `count` entries
    uint64_t count;
    int8_t& i8(int off, int i) { return *reinterpret_cast<int8_t*>(rec.data() + off + i); }
    void i32(int off, int32_t v) { memcpy(rec.data() + off, &v, 4); }
};

static Replica valid_replica() {
    ms_config c{};
    c.n_agents = 3, c.n_cores = 5, c.collection_length = 2, c.n_kinds = 2;
    c.job_priority[0] = 3, c.job_priority[1] = 10, c.job_length[0] = 6, c.job_length[1] = 3;
    c.acc_probability[0] = 0.8, c.acc_probability[1] = 1.0;
    c.free_prices = 1, c.new_jobs_per_round = 1, c.reward_multiplier = 1, c.episode_length = 100, c.liability_cap = 4;
    Replica r;
    r.P = make_params(c, 4);
    const Params& P = r.P;
    r.rec.assign(P.rec_bytes, 0);
    r.i32(0, 17);   // round
    r.i32(8, 300);  // mti
    for (int k = 0; k < P.C; k++) r.i8(P.o_core_owner, k) = 0, r.i8(P.o_core_kind, k) = -1, r.i8(P.o_core_rem, k) = -1;
    r.i8(P.o_core_owner, 0) = 1, r.i8(P.o_core_kind, 0) = 0, r.i8(P.o_core_rem, 0) = 3, r.i8(P.o_liab_n, 0) = 2;
    r.i8(P.o_core_owner, 1) = 2, r.i8(P.o_core_kind, 1) = 1, r.i8(P.o_core_rem, 1) = 1, r.i8(P.o_liab_n, 1) = 1;
    for (int i = 0; i < P.NL; i++) r.i8(P.o_slot_kind, i) = -1, r.i8(P.o_slot_rem, i) = -1, r.i8(P.o_offer_core, i) = -1;
    // agent 1: slot 0 offers its job to core 1 (owner 2), slot 1 free; agent 2: both free; agent 3: one job
    r.i8(P.o_slot_kind, 0) = 0, r.i8(P.o_slot_rem, 0) = 5, r.i8(P.o_slot_wait, 0) = 1;
    r.i8(P.o_offer_core, 0) = 1, r.i8(P.o_offer_recip, 0) = 2, r.i8(P.o_offer_price, 0) = -4;
    r.i8(P.o_slot_kind, 4) = 1, r.i8(P.o_slot_rem, 4) = 2;
    r.liab = {Liab{2, 1, 5, 6, 3}, Liab{3, 2, -2, 1, 9}, Liab{1, 0, 0, 127, 12}};
    r.count = 3;
    return r;
}

static int n_replicas = 0;

static void expect(const char* name, uint32_t code, int index, const std::function<void(Replica&)>& edit) {
    Replica r = valid_replica();
    edit(r);
    r.liab.resize(r.count);  // heap block of exactly count entries
    r.liab.shrink_to_fit();
    const uint32_t f = snap_check_replica(r.P, r.rec.data(), r.liab.data(), r.count);
    n_replicas++;
    if (snap_fail_code(f) != code || (code != kSnapOk && snap_fail_index(f) != index)) {
        printf("FAIL replica %s: got code %u (%s) index %d, want %u (%s) index %d\n", name, snap_fail_code(f),
               snap_code_name(snap_fail_code(f)), snap_fail_index(f), code, snap_code_name(code), index);
        n_fail++;
    }
}

int main() {
    const int shapes[][3] = {{2, 2, 2}, {4, 4, 3}, {8, 8, 3}, {16, 16, 3}, {32, 32, 3}, {1, 1, 16}, {3, 5, 2}, {8, 11, 2}};
    int n_layouts = 0;
    for (const auto& s : shapes)
        for (long long E : {1LL, 2LL, 5LL, 37LL, 4096LL, 16384LL, 300000LL})
            for (long long n : {0LL, 1LL, 2LL, 19LL * E, 32LL * E}) {
                check_layout(s[0], s[1], s[2], E, n);
                n_layouts++;
            }
    const SnapLayout l = snap_layout(16384, make_geom(8, 8, 3, 1).rec_bytes, 19 * 16384);
    printf("layout 8 8 3 16384 %d %llu %llu %llu %llu %llu %llu\n", 19 * 16384, (unsigned long long)l.o_cfg,
           (unsigned long long)l.o_recs, (unsigned long long)l.o_mt, (unsigned long long)l.o_off,
           (unsigned long long)l.o_liab, (unsigned long long)l.total);

    expect("valid", kSnapOk, 0, [](Replica&) {});
    expect("valid, mti 0", kSnapOk, 0, [](Replica& r) { r.i32(8, 0); });
    expect("valid, mti 624", kSnapOk, 0, [](Replica& r) { r.i32(8, 624); });
    expect("valid, full chain", kSnapOk, 0, [](Replica& r) {
        r.i8(r.P.o_liab_n, 0) = 4;
        r.liab.insert(r.liab.begin(), 2, Liab{1, 1, 1, 1, 1});
        r.count = 5;
    });
    expect("mti 700", kSnapMti, 0, [](Replica& r) { r.i32(8, 700); });
    expect("mti -1", kSnapMti, 0, [](Replica& r) { r.i32(8, -1); });
    expect("core kind 9", kSnapCoreKind, 1, [](Replica& r) { r.i8(r.P.o_core_kind, 1) = 9; });
    expect("core kind = K", kSnapCoreKind, 0, [](Replica& r) { r.i8(r.P.o_core_kind, 0) = 2; });
    expect("core kind -2", kSnapCoreKind, 3, [](Replica& r) { r.i8(r.P.o_core_kind, 3) = -2; });
    expect("owner N + 1", kSnapCoreOwner, 0, [](Replica& r) { r.i8(r.P.o_core_owner, 0) = 4; });
    expect("owner -1", kSnapCoreOwner, 2, [](Replica& r) { r.i8(r.P.o_core_owner, 2) = -1; });
    expect("owner 0 with a job", kSnapOwnerEmpty, 1, [](Replica& r) { r.i8(r.P.o_core_owner, 1) = 0; });
    expect("owner of an empty core", kSnapOwnerEmpty, 4, [](Replica& r) { r.i8(r.P.o_core_owner, 4) = 3; });
    expect("remaining length 0", kSnapCoreRem, 0, [](Replica& r) { r.i8(r.P.o_core_rem, 0) = 0; });
    expect("liab_n cap + 1", kSnapLiabN, 1, [](Replica& r) { r.i8(r.P.o_liab_n, 1) = 5; });
    expect("liab_n 255", kSnapLiabN, 4, [](Replica& r) { r.i8(r.P.o_liab_n, 4) = -1; });
    expect("span shorter than the counts", kSnapLiabCount, 0, [](Replica& r) { r.count = 2; });
    expect("span longer than the counts", kSnapLiabCount, 0, [](Replica& r) {
        r.liab.push_back(Liab{1, 1, 1, 1, 1});
        r.count = 4;
    });
    expect("empty span", kSnapLiabCount, 0, [](Replica& r) { r.count = 0; });
    expect("entry offerer 0", kSnapLiabEntry, 0, [](Replica& r) { r.liab[1].offerer = 0; });
    expect("entry offerer N + 1", kSnapLiabEntry, 1, [](Replica& r) { r.liab[2].offerer = 4; });
    expect("entry recipient N + 1", kSnapLiabEntry, 0, [](Replica& r) { r.liab[0].recipient = 4; });
    expect("entry recipient -1", kSnapLiabEntry, 0, [](Replica& r) { r.liab[0].recipient = -1; });
    expect("entry necessary time 0", kSnapLiabEntry, 1, [](Replica& r) { r.liab[2].nec = 0; });
    expect("slot kind 9", kSnapSlotKind, 4, [](Replica& r) { r.i8(r.P.o_slot_kind, 4) = 9; });
    expect("slot remaining length 0", kSnapSlotRem, 0, [](Replica& r) { r.i8(r.P.o_slot_rem, 0) = 0; });
    expect("offer to core C", kSnapOfferCore, 0, [](Replica& r) { r.i8(r.P.o_offer_core, 0) = 5; });
    expect("offer core -2", kSnapOfferCore, 3, [](Replica& r) { r.i8(r.P.o_offer_core, 3) = -2; });
    expect("offer of an empty slot", kSnapOfferCore, 5, [](Replica& r) { r.i8(r.P.o_offer_core, 5) = 0, r.i8(r.P.o_offer_recip, 5) = 1; });
    expect("offer recipient is not the owner", kSnapOfferRecip, 0, [](Replica& r) { r.i8(r.P.o_offer_recip, 0) = 1; });
    expect("offer to an empty core not addressed to the auctioneer", kSnapOfferRecip, 4, [](Replica& r) {
        r.i8(r.P.o_offer_core, 4) = 2, r.i8(r.P.o_offer_recip, 4) = 3;
    });
    expect("agent without a free slot for its core", kSnapFreeSlots, 1, [](Replica& r) {
        r.i8(r.P.o_slot_kind, 1) = 0, r.i8(r.P.o_slot_rem, 1) = 1;
    });
    expect("agent 2 with two cores and one free slot", kSnapFreeSlots, 2, [](Replica& r) {
        r.i8(r.P.o_core_owner, 2) = 2, r.i8(r.P.o_core_kind, 2) = 0, r.i8(r.P.o_core_rem, 2) = 2;
        r.i8(r.P.o_slot_kind, 2) = 1, r.i8(r.P.o_slot_rem, 2) = 1;
    });
    printf("checked %d %d\n", n_layouts, n_replicas);
    return n_fail ? 1 : 0;
}
