// ms_snapshot.h — the packed env snapshot (ms_env_snapshot / ms_env_restore): section offsets and the
// per-replica check, shared by the host ABI (capi.cpp), the kernels (snapshot_kernels.hip) and a host
// program without HIP (tests/snapshot_check.cpp).
//
// One little-endian buffer, every section 16-byte aligned:
//
//   header    64 B            SnapHeader
//   config    sizeof(ms_config), padded to 16: the env's configuration, struct padding zeroed
//   recs      [E][rec_bytes]  the records as they are, header dword 3 (mt_sel) written as 0
//   mt        [E][624] u32    the current MT19937 half of every replica (random.getstate()'s words)
//   liab_off  [E + 1] u64     exclusive prefix sum over replicas of sum_c liab_n[e][c], padded to 16
//   liab      [n_liab] x 8 B  the live ms::Liab entries; within a replica core-major, oldest first
//
// The successor MT half (twist(current)) and the chain slots at or beyond liab_n hold no information and
// are left out.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "ms_layout.h"
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

namespace ms {

constexpr uint32_t kSnapMagic = 0x5053534Du;  // the bytes "MSSP"
constexpr uint32_t kSnapVersion = 1;

struct SnapHeader {
    uint32_t magic, version;
    int64_t E;
    int32_t N, C, L, cap, rec_bytes, cfg_bytes;
    int64_t n_liab;        // live liability entries of all replicas
    uint64_t total_bytes;  // the snapshot's size
    uint32_t reserved[2];
};
static_assert(sizeof(SnapHeader) == 64, "the snapshot header is 64 bytes");

struct SnapLayout {
    uint64_t o_cfg, o_recs, o_mt, o_off, o_liab, total;
};

inline constexpr uint64_t snap_align16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }

// Section offsets of a snapshot of E replicas holding n_liab live entries. Everything before `liab` depends
// on the shape only, so the offsets can be written before the count is known on the host.
inline constexpr SnapLayout snap_layout(int64_t E, int32_t rec_bytes, int64_t n_liab) {
    SnapLayout s{};
    s.o_cfg = sizeof(SnapHeader);
    s.o_recs = snap_align16(s.o_cfg + sizeof(ms_config));
    s.o_mt = s.o_recs + (uint64_t)E * (uint64_t)rec_bytes;  // rec_bytes = align16(..)
    s.o_off = s.o_mt + (uint64_t)E * kMtN * 4;              // 2496 = 156 * 16
    s.o_liab = snap_align16(s.o_off + ((uint64_t)E + 1) * 8);
    s.total = snap_align16(s.o_liab + (uint64_t)n_liab * sizeof(Liab));
    return s;
}

// What the per-replica check refuses (the conditions of ms_env_import's loop, on the packed record).
enum SnapCode : uint32_t {
    kSnapOk = 0,
    kSnapMti,          // mti outside [0, 624]
    kSnapCoreKind,     // core job kind outside [-1, K)
    kSnapCoreOwner,    // core owner outside [0, N]
    kSnapOwnerEmpty,   // owner 0 <=> empty job violated
    kSnapCoreRem,      // a running job's remaining length outside [1, 127]
    kSnapLiabN,        // liab_n > cap
    kSnapLiabCount,    // liab_off[e + 1] - liab_off[e] != sum of the replica's liab_n
    kSnapLiabEntry,    // entry field out of range (offerer [1, N], recipient [0, N], nec [1, 127])
    kSnapSlotKind,     // slot job kind outside [-1, K)
    kSnapSlotRem,      // a waiting job's remaining length outside [1, 127]
    kSnapOfferCore,    // pending offer's core outside [-1, C), or an offer of an empty slot
    kSnapOfferRecip,   // pending offer's recipient is not its core's owner
    kSnapFreeSlots,    // an agent holds fewer free slots than cores
    kSnapLiabOff,      // liab_off decreasing, beyond n_liab, or not starting at 0 / ending at n_liab
    kSnapCodes
};

inline const char* snap_code_name(uint32_t code) {
    const char* names[] = {"ok", "mt_index out of range", "bad core kind", "bad core owner",
                           "owner 0 <=> empty job violated", "bad core remaining length",
                           "liability chain too long (liab_n)", "liab_off span is not the sum of liab_n",
                           "bad liability entry", "bad slot kind", "bad slot remaining length", "bad pending offer",
                           "offer recipient is not the core owner", "fewer free slots than owned cores",
                           "bad liab_off"};
    return code < kSnapCodes ? names[code] : "unknown";
}

// a failure: code in bits 0..7, the core / slot / agent it names in bits 8..23
inline constexpr uint32_t snap_fail(uint32_t code, int32_t index) { return code | ((uint32_t)index << 8); }
inline constexpr uint32_t snap_fail_code(uint32_t f) { return f & 0xffu; }
inline constexpr int32_t snap_fail_index(uint32_t f) { return (int32_t)((f >> 8) & 0xffffu); }

inline constexpr int32_t snap_i8(const uint8_t* rec, int32_t off, int32_t i) { return (int8_t)rec[off + i]; }
inline constexpr int32_t snap_i32(const uint8_t* rec, int32_t off) {
    return (int32_t)((uint32_t)rec[off] | (uint32_t)rec[off + 1] << 8 | (uint32_t)rec[off + 2] << 16 |
                     (uint32_t)rec[off + 3] << 24);
}

// The check of one replica: rec = its packed record (P.rec_bytes readable), liab = its `count` packed
// entries. Reads rec[0, rec_bytes) and liab[0, count) only, whatever they hold. Returns kSnapOk or snap_fail().
inline constexpr uint32_t snap_check_replica(const Params& P, const uint8_t* rec, const Liab* liab, uint64_t count) {
    const int32_t N = P.N, C = P.C, L = P.L, NL = P.NL, K = P.K;
    const int32_t mti = snap_i32(rec, 8);
    if (mti < 0 || mti > kMtN) return snap_fail(kSnapMti, 0);
    uint64_t sum = 0;
    for (int32_t c = 0; c < C; c++) {
        const int32_t k = snap_i8(rec, P.o_core_kind, c), own = snap_i8(rec, P.o_core_owner, c);
        if (k < -1 || k >= K) return snap_fail(kSnapCoreKind, c);
        if (own < 0 || own > N) return snap_fail(kSnapCoreOwner, c);
        if ((k < 0) != (own == 0)) return snap_fail(kSnapOwnerEmpty, c);
        const int32_t rem = snap_i8(rec, P.o_core_rem, c);
        if (k >= 0 && rem < 1) return snap_fail(kSnapCoreRem, c);
        const int32_t n = rec[P.o_liab_n + c];
        if (n > P.cap) return snap_fail(kSnapLiabN, c);
        sum += (uint64_t)n;
    }
    if (sum != count) return snap_fail(kSnapLiabCount, 0);
    uint64_t q = 0;
    for (int32_t c = 0; c < C; c++) {
        const int32_t n = rec[P.o_liab_n + c];
        for (int32_t i = 0; i < n; i++, q++) {
            const Liab& le = liab[q];
            if (le.offerer < 1 || le.offerer > N || le.recipient < 0 || le.recipient > N || le.nec < 1)
                return snap_fail(kSnapLiabEntry, c);
        }
    }
    for (int32_t i = 0; i < NL; i++) {
        const int32_t k = snap_i8(rec, P.o_slot_kind, i);
        if (k < -1 || k >= K) return snap_fail(kSnapSlotKind, i);
        if (k >= 0 && snap_i8(rec, P.o_slot_rem, i) < 1) return snap_fail(kSnapSlotRem, i);
        const int32_t oc = snap_i8(rec, P.o_offer_core, i);
        if (oc < -1 || oc >= C || (oc >= 0 && k < 0)) return snap_fail(kSnapOfferCore, i);
        // offers to a core are addressed to its owner (world.py:428 runs after the tick)
        if (oc >= 0 && snap_i8(rec, P.o_offer_recip, i) != snap_i8(rec, P.o_core_owner, oc))
            return snap_fail(kSnapOfferRecip, i);
    }
    for (int32_t a = 0; a < N; a++) {  // numberOfFreeSlots >= len(ownedCores) (world.py:371-373 keeps it)
        int32_t owned = 0, empty = 0;
        for (int32_t c = 0; c < C; c++) owned += snap_i8(rec, P.o_core_owner, c) == a + 1;
        for (int32_t l = 0; l < L; l++) empty += snap_i8(rec, P.o_slot_kind, a * L + l) < 0;
        if (empty < owned) return snap_fail(kSnapFreeSlots, a + 1);
    }
    return kSnapOk;
}

// launch arguments of the snapshot kernels
struct SnapArgs {
    uint8_t* recs;    // the env's [E][rec_bytes]
    uint32_t* mt;     // [E][2][624]
    Liab* liab;       // [E][C][cap]
    uint8_t* buf;     // the snapshot
    uint64_t bytes;   // its size (validate: every offset followed stays below it)
    SnapLayout lay;
    int64_t E, n_liab;
};


#ifdef __HIPCC__  // the launchers of snapshot_kernels.hip (everything above needs no HIP: tests/snapshot_check.cpp)
// The whole pack, or the count alone (a.buf NULL); *total (host-coherent) = n_liab once the stream has run
hipError_t launch_snap_pack(const Params& P, const SnapArgs& a, const SnapHeader& h, const uint8_t* cfg_bytes,
                            uint64_t* total, hipStream_t st);
// the snapshot's sections back into the env's arrays (validated first: launch_snap_validate)
hipError_t launch_snap_unpack(const Params& P, const SnapArgs& a, hipStream_t st);
// result[0]: the first failing (replica << 24 | failure), ~0 for none; result[1]: the OR of the records' flags
hipError_t launch_snap_validate(const Params& P, const SnapArgs& a, unsigned long long* result, hipStream_t st);
#endif

}  // namespace ms
