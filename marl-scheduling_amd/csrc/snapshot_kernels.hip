// snapshot_kernels.hip — pack, validate and unpack of the env snapshot (ms_snapshot.h).
//
// A snapshot keeps what the env's state holds as information: the records, the current MT19937 half and the
// live liability entries (cfg3: ~2.9 KB of a replica's 13.5 KB). Packing is three launches on one stream:
//   k_snap_bulk     one wave per replica: record and MT half with 16-byte loads and stores (both are whole
//                   multiples of 16 B), and the replica's number of live entries into liab_off[e];
//   k_snap_offsets  one workgroup: exclusive scan of the counts in place, the header, the pad bytes, the total
//                   into host-coherent memory (alone, reading the records, it only counts);
//   k_snap_entries  one wave per replica: a lane per live entry, 8-byte copies into the replica's span.
// Restoring is k_snap_validate (reads the snapshot only), then k_snap_unpack.
#include <hip/hip_runtime.h>

#include <string.h>

#include "ms_snapshot.h"

namespace ms {

namespace {

constexpr int kScanThreads = 1024;
constexpr int kScanPer = 8;        // replicas per thread and chunk
constexpr int kCopyThreads = 256;  // 4 waves = 4 replicas per workgroup
constexpr int kMt16 = kMtN / 4;    // 156 16-byte pieces = 64 + 64 + 28
static_assert(kMt16 > 2 * kWave && kMt16 <= 3 * kWave, "the MT half is three pieces per lane");

// live entries of replica e: the sum of its liab_n bytes
__device__ __forceinline__ uint32_t replica_count(const uint8_t* rec, const Geom& P) {
    uint32_t n = 0;
    for (int c = 0; c < P.C; c++) n += rec[P.o_liab_n + c];
    return n;
}

__device__ __forceinline__ int64_t wave_replica() {
    return (int64_t)blockIdx.x * (kCopyThreads / kWave) + threadIdx.x / kWave;
}

// dst record := src record with header dword 3 (mt_sel) written as 0; dst MT half := src MT half. The loads
// of the MT half are issued before its stores.
__device__ __forceinline__ void copy_record_and_mt(uint4* __restrict__ rec_dst, const uint4* __restrict__ rec_src,
                                                   int rec16, uint4* __restrict__ mt_dst,
                                                   const uint4* __restrict__ mt_src, int lane) {
    const uint4 m0 = mt_src[lane], m1 = mt_src[lane + kWave];
    uint4 m2{};
    if (lane < kMt16 - 2 * kWave) m2 = mt_src[lane + 2 * kWave];
    for (int i = lane; i < rec16; i += kWave) {
        uint4 v = rec_src[i];
        if (i == 0) v.w = 0u;
        rec_dst[i] = v;
    }
    mt_dst[lane] = m0;
    mt_dst[lane + kWave] = m1;
    if (lane < kMt16 - 2 * kWave) mt_dst[lane + 2 * kWave] = m2;
}

// One wave per replica: record, current MT half (the record's dword 3 selects it), count. Needs a buffer that
// holds the sections before the entries (a.bytes >= a.lay.o_liab).
__global__ __launch_bounds__(kCopyThreads) void k_snap_bulk(Params P, SnapArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t e = wave_replica();
    if (e >= a.E) return;
    const uint8_t* rec = a.recs + e * P.rec_bytes;
    const uint32_t sel = *reinterpret_cast<const uint32_t*>(rec + 12) & 1u;
    uint32_t n = lane < P.C ? rec[P.o_liab_n + lane] : 0u;  // C <= 64
    copy_record_and_mt(reinterpret_cast<uint4*>(a.buf + a.lay.o_recs + (uint64_t)e * P.rec_bytes),
                       reinterpret_cast<const uint4*>(rec), P.rec_bytes / 16,
                       reinterpret_cast<uint4*>(a.buf + a.lay.o_mt + (uint64_t)e * kMtN * 4),
                       reinterpret_cast<const uint4*>(a.mt + ((uint64_t)e * 2 + sel) * kMtN), lane);
    for (int d = kWave / 2; d > 0; d >>= 1) n += (uint32_t)__shfl_xor((int)n, d);
    if (lane == 0) reinterpret_cast<uint64_t*>(a.buf + a.lay.o_off)[e] = n;
}

// liab_off[e] = sum of the counts of replicas < e, liab_off[E] = *total = n_liab. One workgroup walks E in
// chunks of kScanThreads * kScanPer replicas: a thread takes kScanPer consecutive replicas (their loads in
// flight together), the workgroup scans the threads' sums. With a buffer (a.buf; its liab_off holds the counts,
// k_snap_bulk) the scan is in place, each thread writing the elements it read, and the kernel also writes
// what does not depend on the records: the header and the config (head, n_liab and total_bytes filled in here)
// and the pad bytes behind liab_off and behind the last entry, the latter only where a.bytes (the buffer's
// capacity) holds it. a.buf == NULL: the counts come from the records and only *total (host-coherent memory) is
// written.
struct SnapHead {
    SnapHeader h;
    uint8_t cfg[sizeof(ms_config)];
};

__global__ __launch_bounds__(kScanThreads) void k_snap_offsets(Params P, SnapArgs a, SnapHead head, uint64_t* total) {
    __shared__ uint32_t part[kScanThreads / kWave];
    __shared__ uint64_t running;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    const int64_t E = a.E;
    uint64_t* off = a.buf ? reinterpret_cast<uint64_t*>(a.buf + a.lay.o_off) : nullptr;
    if (tid == 0) running = 0;
    __syncthreads();
    for (int64_t e0 = 0; e0 < E; e0 += (int64_t)kScanThreads * kScanPer) {
        const int64_t e = e0 + (int64_t)tid * kScanPer;
        uint32_t n[kScanPer], mine = 0;
#pragma unroll
        for (int i = 0; i < kScanPer; i++) {
            n[i] = 0u;
            if (e + i < E) n[i] = off ? (uint32_t)off[e + i] : replica_count(a.recs + (e + i) * P.rec_bytes, P);
        }
#pragma unroll
        for (int i = 0; i < kScanPer; i++) mine += n[i];
        uint32_t incl = mine;  // inclusive scan in the wave
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == kWave - 1) part[w] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int i = 0; i < kScanThreads / kWave; i++) {
            const uint32_t p = part[i];
            before += i < w ? p : 0u;
            all += p;
        }
        const uint64_t base = running;
        if (off) {
            uint64_t o = base + before + (incl - mine);
#pragma unroll
            for (int i = 0; i < kScanPer; i++) {
                if (e + i < E) off[e + i] = o;
                o += n[i];
            }
        }
        __syncthreads();  // every thread has read running and part
        if (tid == 0) running = base + all;
        __syncthreads();
    }
    const uint64_t n_liab = running;
    const SnapLayout lay = snap_layout(E, P.rec_bytes, (int64_t)n_liab);
    if (off) {  // (the capacity holds everything up to o_liab)
        const uint8_t* src = reinterpret_cast<const uint8_t*>(&head);
        for (uint32_t i = tid; i < lay.o_recs; i += kScanThreads) a.buf[i] = i < sizeof(SnapHead) ? src[i] : (uint8_t)0;
        __syncthreads();
        if (tid == 0) {
            static_assert(offsetof(SnapHeader, n_liab) == 40 && offsetof(SnapHeader, total_bytes) == 48, "header fields");
            reinterpret_cast<uint64_t*>(a.buf)[5] = n_liab;
            reinterpret_cast<uint64_t*>(a.buf)[6] = lay.total;
            off[E] = n_liab;
            if (lay.o_off + ((uint64_t)E + 1) * 8 < lay.o_liab) off[E + 1] = 0;  // liab_off's pad
            const uint64_t end = lay.o_liab + n_liab * sizeof(Liab);
            if (end < lay.total && lay.total <= a.bytes) *reinterpret_cast<uint64_t*>(a.buf + end) = 0;  // the entries' pad
        }
    }
    if (tid == 0) {
        *total = n_liab;
        __threadfence_system();
    }
}

// The live entries of one replica between its chains [C][cap] and its packed span (core-major, oldest first), by
// one wave: lane c holds liab_n[c] (n, clamped to cap) and the wave finds, for the packed index i of each lane,
// the core whose entries cover it. kPack: chains -> span, else span -> chains.
template <bool kPack>
__device__ __forceinline__ void copy_entries(uint64_t* __restrict__ chains, uint64_t* __restrict__ span, uint32_t n,
                                             int C, int cap, int lane) {
    uint32_t incl = n;
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
        if (lane >= d) incl += up;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, kWave - 1);
    for (uint32_t i0 = 0; i0 < total; i0 += kWave) {  // (wave-uniform trip count)
        const uint32_t i = i0 + lane;
        uint32_t c = 0, base = 0;
        for (int j = 0; j < C; j++) {
            const uint32_t end = (uint32_t)__shfl((int)incl, j);
            if (end <= i) c = j + 1, base = end;
        }
        if (i < total) {  // then c < C and i - base < n[c] <= cap
            uint64_t* slot = chains + (uint64_t)c * cap + (i - base);
            if (kPack) span[i] = *slot;
            else *slot = span[i];
        }
    }
}

// One wave per replica: its live entries into [liab_off[e], liab_off[e] + count), where the capacity holds the
// span (the launch precedes the host's look at the count: a buffer that proves too small is refused afterwards,
// and nothing is written beyond it).
__global__ __launch_bounds__(kCopyThreads) void k_snap_entries(Params P, SnapArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t e = wave_replica();
    if (e >= a.E) return;
    const uint8_t* rec = a.recs + e * P.rec_bytes;
    const uint64_t* off = reinterpret_cast<const uint64_t*>(a.buf + a.lay.o_off);
    const uint64_t first = off[e], count = off[e + 1] - first;
    uint32_t n = lane < P.C ? rec[P.o_liab_n + lane] : 0u;
    if (a.lay.o_liab + (first + count) * sizeof(Liab) > a.bytes) return;
    // (a chain longer than cap, which no round leaves behind, would be read up to cap: its span keeps the
    // count, and ms_env_restore refuses such a record)
    n = n < (uint32_t)P.cap ? n : (uint32_t)P.cap;
    copy_entries<true>(reinterpret_cast<uint64_t*>(a.liab + (uint64_t)e * P.C * P.cap),
                       reinterpret_cast<uint64_t*>(a.buf + a.lay.o_liab) + first, n, P.C, P.cap, lane);
}

// The inverse of the pack, after validation: the record as it is (mt_sel = 0: the current block is half 0, the
// device recomputes its successor before the replica's next draw), the MT block into half 0, the entries
// into their chains (slots at or beyond liab_n are not written: nothing reads them).
__global__ __launch_bounds__(kCopyThreads) void k_snap_unpack(Params P, SnapArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t e = wave_replica();
    if (e >= a.E) return;
    const uint8_t* rec = a.buf + a.lay.o_recs + (uint64_t)e * P.rec_bytes;
    const uint32_t n = lane < P.C ? rec[P.o_liab_n + lane] : 0u;  // <= cap (validated)
    copy_record_and_mt(reinterpret_cast<uint4*>(a.recs + e * P.rec_bytes), reinterpret_cast<const uint4*>(rec),
                       P.rec_bytes / 16, reinterpret_cast<uint4*>(a.mt + (uint64_t)e * 2 * kMtN),
                       reinterpret_cast<const uint4*>(a.buf + a.lay.o_mt + (uint64_t)e * kMtN * 4), lane);
    const uint64_t first = reinterpret_cast<const uint64_t*>(a.buf + a.lay.o_off)[e];
    copy_entries<false>(reinterpret_cast<uint64_t*>(a.liab + (uint64_t)e * P.C * P.cap),
                        reinterpret_cast<uint64_t*>(a.buf + a.lay.o_liab) + first, n, P.C, P.cap, lane);
}

// One lane per replica applies snap_check_replica to the snapshot alone. The host has checked the header, so
// the fixed sections lie inside [buf, buf + bytes) (lay.total == bytes); the only offsets read from the buffer
// are liab_off[e] and liab_off[e + 1], and they are range-checked against n_liab before any entry is read.
// result[0]: the smallest (replica << 24 | failure) of the failing replicas (min: the report does not depend on
// the order the lanes run in); result[1]: the OR of the records' flags.
__global__ __launch_bounds__(kCopyThreads) void k_snap_validate(Params P, SnapArgs a, unsigned long long* result) {
    const int64_t e = (int64_t)blockIdx.x * kCopyThreads + threadIdx.x;
    if (e >= a.E) return;
    const uint8_t* rec = a.buf + a.lay.o_recs + (uint64_t)e * P.rec_bytes;
    const uint64_t* off = reinterpret_cast<const uint64_t*>(a.buf + a.lay.o_off);
    const uint64_t lo = off[e], hi = off[e + 1], n_liab = (uint64_t)a.n_liab;
    uint32_t f;
    if (lo > hi || hi > n_liab || (e == 0 && lo != 0) || (e == a.E - 1 && hi != n_liab) ||
        a.lay.o_liab + hi * sizeof(Liab) > a.bytes) {
        f = snap_fail(kSnapLiabOff, 0);
    } else {
        f = snap_check_replica(P, rec, reinterpret_cast<const Liab*>(a.buf + a.lay.o_liab) + lo, hi - lo);
    }
    if (f != kSnapOk) atomicMin(&result[0], ((unsigned long long)e << 24) | f);
    const uint32_t flags = *reinterpret_cast<const uint32_t*>(rec + 4);
    if (flags) atomicOr(&result[1], (unsigned long long)flags);
}

dim3 wave_grid(int64_t E) {
    const int per = kCopyThreads / kWave;
    return dim3((unsigned)((E + per - 1) / per));
}

}  // namespace

// The whole pack, or the count alone. a.buf: the buffer, or NULL to count only; a.bytes: its capacity, at least
// a.lay.o_liab; a.lay: the layout without entries (the sections before them depend on the shape only).
// *total (host-coherent) = n_liab once the stream has run.
hipError_t launch_snap_pack(const Params& P, const SnapArgs& a, const SnapHeader& h, const uint8_t* cfg_bytes,
                            uint64_t* total, hipStream_t st) {
    SnapHead head{};
    head.h = h;
    memcpy(head.cfg, cfg_bytes, sizeof(head.cfg));
    if (a.buf) hipLaunchKernelGGL(k_snap_bulk, wave_grid(a.E), dim3(kCopyThreads), 0, st, P, a);
    hipLaunchKernelGGL(k_snap_offsets, dim3(1), dim3(kScanThreads), 0, st, P, a, head, total);
    if (a.buf) hipLaunchKernelGGL(k_snap_entries, wave_grid(a.E), dim3(kCopyThreads), 0, st, P, a);
    return hipGetLastError();
}

hipError_t launch_snap_unpack(const Params& P, const SnapArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_snap_unpack, wave_grid(a.E), dim3(kCopyThreads), 0, st, P, a);
    return hipGetLastError();
}

hipError_t launch_snap_validate(const Params& P, const SnapArgs& a, unsigned long long* result, hipStream_t st) {
    hipLaunchKernelGGL(k_snap_validate, dim3((unsigned)((a.E + kCopyThreads - 1) / kCopyThreads)), dim3(kCopyThreads),
                       0, st, P, a, result);
    return hipGetLastError();
}

}  // namespace ms
