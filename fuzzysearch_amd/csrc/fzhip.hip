// fzhip.hip — host side of libfzhip.so: the C-ABI of include/fzhip.h over the gfx950 kernels.
//
// Data layout in HBM (per device shard):
//   [FZ_PAD_FRONT zero bytes][buf_len sequence bytes][zero bytes up to a whole tile + FZ_PAD_BACK]
// so the scan can read whole 16 KiB tiles and 8-byte halos without bounds checks; zero padding can
// never create an accepted hit because every candidate is range-checked against the global length.
//   d_out  : [1 KiB header: counters][records, 24 B each] in one allocation, so the usual result
//            comes back in ONE D2H copy (header + about as many records as the previous call had)
//              counters[0]      hits emitted to d_hits (non-fused paths)
//              counters[1]      records written
//              counters[2]      automaton work items whose candidate lists overflowed
//              counters[8..71]  confirmed n-gram hits of the fused scan (64 words: one word only
//                               sustains ~90 atomics/us)
//   d_hits : uint64 (block << 56 | global idx) hit list — only the non-fused paths use it
// The GPU produces records unordered; the host puts them in the reference's emission order by a radix
// sort on (block, idx) — the number of records is tiny next to the bytes scanned.
// Every search is synchronous: when a fz_* call returns its results are on the host and nothing is
// in flight on the sequence.  Buffers that turn out too small are grown and the search re-runs.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>                             // types only: the library is dlopen-ed on first use (rccl_api)
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <thread>
#include <unistd.h>
#include <map>
#include <mutex>
#include <vector>
#include <cassert>

#include "../../include/fzhip.h"
#include "fz_kernels.h"

namespace {

// Every process-wide switch of the library: read from the environment ONCE, on first use, into this struct.  None of them is
// needed to use the library; tests and A/B measurements set them (INTEGRATION.md §5 describes each).  Results never depend
// on a switch — the -m gpu suite runs the same cases under the ones marked (t) and compares with the oracle.
struct Switches {
    // (t) alternative forms of the same computation
    bool no_direct = false;            // FZ_NO_DIRECT: records / counters through D2H copies, never the kernels' stores into pinned memory
    bool no_slot_and = false;          // FZ_NO_SLOT_AND: the filter's general slot form (shift + and) for every launch
    int max_blocks = 0;                // FZ_MAX_BLOCKS=n: at most n n-gram blocks per scan launch
    bool force_big_verify = false;     // FZ_FORCE_BIG_VERIFY: every stand-alone verification by fz_verify_big_kernel
    bool no_wf_fuse = false;           // FZ_NO_WF_FUSE: budgets 5 .. 15 verified by the stand-alone kernel, not inside the scan
    int wf32 = -1;                     // FZ_WF32=0 / 1: pin the fused lane-per-cell form off / on for budgets 8 .. 15 (default: by density)
    bool no_bits = false;              // FZ_NO_BITS: no bit-vector verification (Levenshtein budgets >= FZ_BITS_MIN_K take round 5's forms)
    int bits_min_k = 3;                // FZ_BITS_MIN_K=k: smallest Levenshtein budget always verified by bit-vector columns (below: the register
                                       // band unless the pattern lets expect dense candidates)
    int bits_qcap = 0;                 // FZ_BITS_QCAP=n: queue entries per wave of the bit-vector form (default: by LDS)
    bool gen_legacy = false;           // FZ_GEN_LEGACY: the generic automaton as fz_lp_kernel (one wave per hit, round 3's form)
    bool gen_no_dedup = false;         // FZ_GEN_NO_DEDUP: no window table (every n-gram hit runs its automaton)
    int gh_waves = 0;                  // FZ_GH_WAVES=1 / 2 / 4: waves per hit of fz_gen_hit_kernel
    bool gh_no_bits = false;           // FZ_GH_NO_BITS: round 4's candidate step instead of the bit-parallel one
    int cand_lds_max = 0;              // FZ_CAND_LDS_MAX=n: candidate lists beyond n entries live in HBM
    bool mp_force_pass = false;        // FZ_MP_FORCE_PASS: every multi-pattern group of two or more rides a pass, whatever the cost rule expects
                                       // (how benchmarks/multi_pattern.py measures the cells the rule gives to the loop)
    bool no_dev_threads = false;       // FZ_NO_DEV_THREADS: a multi-device context drives every device from the calling thread
    int taper_steps = 4;               // FZ_TAPER_STEPS (0: no regions), FZ_TAPER_MIN, FZ_TAPER_WG_PER_CU: the scan grid's last round
    double taper_min = 0.25;
    int taper_wg_per_cu = 7;
    int scan_dir = 0;                  // FZ_SCAN_DIR=alt / fwd / rev: a context's default for fz_set_scan_direction (0 alternate, 1 always
                                       // forward, 2 always reversed)
    bool scan_rounds = false;          // FZ_SCAN_ROUNDS=1: a scan next to its predecessor lays its first and last resident round down in
                                       // address order (plan_scan_rounds; measured, not the default: profiles/r25_sweep_direction.txt)
    bool no_rccl = false;              // FZ_NO_RCCL: behave like an install without librccl
    std::string rccl_lib;              // FZ_RCCL_LIB=path: the collective library to dlopen first (tests: tests/libmock_rccl.so)
    std::string rocm_path = "/opt/rocm";   // ROCM_PATH
    long comm_timeout_ms = 60000;      // FZ_COMM_TIMEOUT_MS: deadline of every wait for a collective (then FZ_ETIMEOUT, not a hung job)
    // diagnostics (print only)
    bool trace = false;                // FZ_TRACE: per-phase host timings of a search on stderr
    bool stream_trace = false;         // FZ_STREAM_TRACE: host time split of a file stream on stderr
};

Switches read_switches() {
        Switches v;
        auto flag = [](const char *n) { return getenv(n) != nullptr; };
        auto num = [](const char *n, int dflt) { const char *e = getenv(n); return e ? atoi(e) : dflt; };
        v.no_direct = flag("FZ_NO_DIRECT"); v.no_slot_and = flag("FZ_NO_SLOT_AND"); v.max_blocks = num("FZ_MAX_BLOCKS", 0);
        v.force_big_verify = flag("FZ_FORCE_BIG_VERIFY"); v.no_wf_fuse = flag("FZ_NO_WF_FUSE");
        v.no_bits = flag("FZ_NO_BITS"); v.bits_min_k = num("FZ_BITS_MIN_K", 3); v.bits_qcap = num("FZ_BITS_QCAP", 0);
        v.wf32 = num("FZ_WF32", -1); v.gen_legacy = flag("FZ_GEN_LEGACY"); v.gen_no_dedup = flag("FZ_GEN_NO_DEDUP");
        v.gh_waves = num("FZ_GH_WAVES", 0); v.gh_no_bits = flag("FZ_GH_NO_BITS"); v.cand_lds_max = num("FZ_CAND_LDS_MAX", 0);
        v.no_dev_threads = flag("FZ_NO_DEV_THREADS"); v.taper_steps = num("FZ_TAPER_STEPS", 4);
        if (const char *e = getenv("FZ_TAPER_MIN")) v.taper_min = atof(e);
        v.taper_wg_per_cu = num("FZ_TAPER_WG_PER_CU", 7); v.no_rccl = flag("FZ_NO_RCCL");
        if (const char *e = getenv("FZ_RCCL_LIB")) v.rccl_lib = e;
        if (const char *e = getenv("ROCM_PATH")) v.rocm_path = e;
        if (const char *e = getenv("FZ_COMM_TIMEOUT_MS")) v.comm_timeout_ms = std::max(1L, atol(e));
        v.mp_force_pass = flag("FZ_MP_FORCE_PASS");
        if (const char *e = getenv("FZ_SCAN_DIR")) v.scan_dir = !strcmp(e, "fwd") ? 1 : !strcmp(e, "rev") ? 2 : 0;
        v.scan_rounds = flag("FZ_SCAN_ROUNDS");
        v.trace = flag("FZ_TRACE"); v.stream_trace = flag("FZ_STREAM_TRACE");
        return v;
}

Switches &switches_storage() { static Switches s = read_switches(); return s; }
const Switches &sw() { return switches_storage(); }

// FZ_TRACE=1: per-phase host timings of a search call on stderr (tuning aid)
struct Trace {
    bool on;
    std::chrono::steady_clock::time_point t0, last;
    Trace() : on(sw().trace) { t0 = last = std::chrono::steady_clock::now(); }
    void mark(const char *what) {
        if (!on) return;
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[fz] %-18s %8.1f us (total %8.1f)\n", what,
                std::chrono::duration<double, std::micro>(now - last).count(),
                std::chrono::duration<double, std::micro>(now - t0).count());
        last = now;
    }
};

thread_local std::string g_err;

// FZ_NO_DIRECT=1 (test / lab knob): records and counters always come back through a D2H copy, never by the kernels' own
// stores into the pinned staging buffer
bool env_no_direct() { return sw().no_direct; }

int fail(int code, const char *fmt, ...) {
    char tmp[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(tmp, sizeof tmp, fmt, ap);
    va_end(ap);
    g_err = tmp;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? FZ_ENOMEM : FZ_EDEVICE, "%s failed: %s", #expr, \
                        hipGetErrorString(e_));                                                    \
    } while (0)

constexpr uint64_t kHeaderBytes = 1024;          // counters[0] = emitted hits, [1] = records, [8..71] = confirmed-hit tallies
constexpr uint64_t kFirstCopyRecs = 4096;        // records fetched together with the header
constexpr uint64_t kHostRecs = 16384;            // records the pinned staging buffer holds (direct mode)
static_assert(kHeaderBytes == FZ_HDR_WORDS * 8, "header layout");

// What one enqueue decided and the collection of that search needs to know, kept in the result slot the search was launched
// into.  Writers: enqueue_shard (starts from a fresh record) and the launch half of run_generic.  Readers: collect_shard, the
// collect half of run_generic, search_enqueue (form_used, launches_used) and emit_matches (fused_used).
struct SearchRun {
    bool last_direct = false;                    // mode of the search being collected
    bool timed = true;                           // the search being collected recorded its start event
    bool fused_used = false;
    uint32_t form_used = 0;                      // FZ_FORM_* of the last enqueue
    uint32_t launches_used = 0;                  // scan launches of the last enqueue on this device
    bool verify_launched = false;                // the last enqueue ran fz_verify_kernel (ev[2] recorded)
    int scan_end_event = 1;                      // which event marks the end of the last scan (1 or 3)
    int verify_end_event = 2;                    // ... and of the verification kernel behind it (2, or 3 = the completion event)
    bool on_alt = false;                         // the search of this result slot scans on stream_alt (DevState)
    // what the search being collected ran with (an overflow is judged against these, not against buffers
    // that a search collected in between may have grown)
    uint64_t hit_cap_used = 0, rec_cap_used = 0;
    // the generic search (run_generic; in flight it has a lane to itself, not a slot)
    bool dedup_used = false;                     // the search being collected ran with the window table (row count = counters[FZ_HDR_GEN_ROWS])
    bool gen_multi_used = false;                 // ... and its automaton as fz_gen_hit_kernel (counters[FZ_HDR_GEN_FAIL]: hits it gave up on)
    bool fold_was_direct = false;                // mode of the folded search being collected
    uint64_t fold_copied = 0;                    // folded generic search: pairs fetched with the counters
    int lp_end_event = 2;                        // which event marks the end of the last automaton kernel (2, or 3 = the completion)
};

// One result slot of a device state: where a search's counters and records arrive, the events around its kernels, and
// what it ran with.  A device state has two: fz_lev_ngrams_begin with one search already in flight launches into the
// second, so that the host orders the records of search i while search i + 1 scans (two-deep pipeline).
struct ResultSlot {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    uint8_t *h_stage = nullptr;                  // pinned, kHeaderBytes + kHostRecs * sizeof(FzRec)
    uint8_t *h_stage_dev = nullptr;              // the same memory as the device addresses it
    uint8_t *d_send = nullptr;                   // RCCL (fz_comm_*): the snapshot of a collective search's counters + records (DevState::comm)
    hipEvent_t ev_snap = nullptr;                // ... recorded behind the copy that takes it
    bool snap_taken = false;                     // ... and a search has taken one into this slot (ev_snap was recorded)
    SearchRun run;
};

struct DevState {
    int device = 0;
    hipStream_t stream = nullptr;
    ResultSlot slots[2];
    int slot_id = 0;                             // which of the two result slots is the current one
    ResultSlot &cur() { return slots[slot_id]; }
    const ResultSlot &cur() const { return slots[slot_id]; }
    void swap_slot() { slot_id ^= 1; }
    uint64_t *d_hits = nullptr;
    uint64_t hit_cap = 0;
    uint8_t *d_out = nullptr;                    // [header kHeaderBytes][recs]
    uint64_t rec_cap = 0;
    // Direct mode: the kernels write records and (last workgroup) the counters straight into the slot's h_stage,
    // no D2H copy command.  Left when a search produces more than kHostRecs records, re-entered when
    // the counts are small again.
    bool direct = true;
    // Large record sets of the automaton kernels (10^5 .. 10^6 records): a pinned, device-mapped host
    // buffer that grows on demand; the kernel's stores cross PCIe while it runs instead of a D2H copy
    // into pageable memory afterwards.
    uint8_t *d_cand = nullptr;                   // HBM candidate lists of the automaton kernels (rare fallback)
    uint64_t cand_bytes = 0;
    // generic search ordered on the device: per-hit {first row, row count} and the finished fz_match rows
    uint8_t *d_gen_order = nullptr;
    uint8_t *d_gen_rows = nullptr;
    uint8_t *d_gen_dedup = nullptr;               // window table of the generic search (FzGenDedup, fz_device.h)
    bool dedup_zeroed = false;                   // ... zeroed behind the last search that used it
    uint64_t gen_dedup_arg = 0;                  // ... its address for the kernels of the search being launched (0: no table)
    uint64_t gen_rows_cap = 0;                   // rows
    uint8_t *h_big = nullptr;
    uint64_t big_cap = 0;                        // records
    // one recycled sequence allocation (chunked file reads upload / release 1 MiB buffers in a loop;
    // hipMalloc + hipFree per chunk would dominate)
    uint8_t *spare_alloc = nullptr;
    uint64_t spare_bytes = 0;
    hipEvent_t rec_ev[10] = {};                  // fz_batch_upload_records, _fasta: the spans of its copy and kernels (created on first use)
    uint64_t first_copy = 512;                   // records fetched with the header (tracks the last count)
    bool header_zeroed = false;                  // the counters were already zeroed after the last D2H copy
    // staging of the last closed file stream, kept for the next one (pinning 2 x 65 MiB costs ~30 ms)
    uint8_t *stream_h[2] = {nullptr, nullptr};
    uint8_t *stream_d = nullptr;
    uint64_t stream_cap = 0, stream_d_bytes = 0;
    int n_cus = 256;
    double last_filter_ms = 0;                   // scan span of the search collected last on this device (fz_device_ms)
    uint64_t fold_guess = 8192;                  // folded generic search: pairs to fetch with the counters (tracks the last count)
    bool fold_direct = true;                     // ... or written straight into h_stage by the automaton kernel (while they fit)
    uint8_t *d_pat = nullptr;                    // pattern in HBM (subsequences longer than FZ_MAX_M, fz_verify_big_kernel)
    uint64_t pat_cap = 0;
    // multi-pattern search (fz_lev_ngrams_multi): the group descriptor and the counters (fixed sizes, allocated on first use),
    // FZ_MP_LISTS hit lists of mp_hit_cap entries each and mp_rec_cap records — buffers of their own, so that nothing the
    // single-pattern searches keep between calls (zeroed headers, result slots, the direct mode) is touched
    uint8_t *d_mp_desc = nullptr, *d_mp_ctr = nullptr, *d_mp_hits = nullptr, *d_mp_recs = nullptr;
    uint64_t mp_hit_cap = 0, mp_rec_cap = 0;
    uint32_t mp_desc_words = 0;        // dwords of d_mp_desc (a class group's descriptor is longer: it grows for those only)
    // fz_batch_assign: the call's tables and output rows (lo, hi, rows, pattern lengths, aux table: assign_ensure), and the
    // records of a pattern searched on its own on their way to the fold; both grow and stay, like the buffers above
    uint8_t *d_assign = nullptr, *d_assign_recs = nullptr;
    uint64_t assign_cap = 0, assign_rec_cap = 0;
    // Two fused searches in flight: the younger one's scan on the stream the older one does not use, so that it starts
    // while the older scan drains instead of behind it (fz_ctx::streams; enqueue_shard states why the two may share the
    // device).  stream_alt has a counter block of its own; SearchRun::on_alt says which search scans there.
    hipStream_t stream_alt = nullptr;
    uint8_t *d_hdr_alt = nullptr;
    // RCCL (fz_comm_*): this device state is rank comm_rank of a communicator.  A search of such a context leaves
    // its counters + records in d_out; a device-to-device snapshot (the slot's d_send, taken on the scan stream right
    // behind the kernels, so a younger search may reuse d_out) is what the all-gather sends.
    ncclComm_t comm = nullptr;
    int comm_rank = -1;
    hipStream_t comm_stream = nullptr;           // default priority: the collective runs next to the (low-priority) scan
    uint64_t send_cap = 0;                       // records a snapshot holds
    uint8_t *d_recv = nullptr, *h_recv = nullptr;
    uint64_t recv_bytes = 0;
    hipEvent_t ev_done = nullptr;
};

// The events around a search's kernels: the scan (f), the kernel behind it (v), the whole (t); read on demand (fz_ctx::tref).
struct TimingRef { DevState *d; hipEvent_t f0, f1, v0, v1, t0, t1; };
// The timing reference of the search in the device's current slot.  `generic`: the kernel behind the scan is the
// automaton of run_generic, else the stand-alone verification (none: no span).
TimingRef timing_ref(DevState &d, bool generic) {
    const ResultSlot &s = d.cur();
    hipEvent_t v0 = generic || s.run.verify_launched ? s.ev[1] : nullptr;
    return {&d, s.ev[0], s.ev[s.run.scan_end_event], v0, s.ev[generic ? s.run.lp_end_event : s.run.verify_end_event], s.ev[0], s.ev[3]};
}

// A batch of sequences (fz_batch_upload): unsegmented to the planner, the tables in the segment fields (fz_device.h).
inline bool geom_is_ragged(const FzGeom &g) { return g.seg_stride == 0 && g.seg_j1 != 0; }

struct Shard {
    int dev = 0;                                 // index into ctx->devs
    uint8_t *d_alloc = nullptr;                  // allocation base
    uint8_t *d_buf = nullptr;                    // = d_alloc + FZ_PAD_FRONT
    uint64_t alloc_bytes = 0;
    FzGeom geom{};
    // The last launch over this shard's whole buffer walked forward, i.e. towards the physical end (eligible or not; a
    // has_near_match_* launch that skipped tiles counts as well: the bit steers, it promises nothing): the next eligible
    // launch of an alternating context starts at the end and walks back (enqueue_shard).  Launch state, not data: mutable.
    mutable bool scan_at_end = false;
};

}  // namespace

namespace {

// One host thread per device of a multi-device context (round 4).  A search over N shards used to be driven by the
// calling thread alone: N x ~10 us of launches one after the other, N waits, and the ordering of all N record lists
// (8 x 10^4 records at N = 8: 0.35 ms) against a 0.79 ms kernel.  Every device's worker now enqueues, waits for,
// collects AND orders its own shard; the caller only merges the ordered rows block by block.  Workers spin for a
// while after a job (the next one of a pipelined loop arrives within a millisecond), then sleep on a condition variable.
// FZ_NO_DEV_THREADS=1: no workers, the calling thread does everything in shard order (A/B knob).
struct DevWorkers {
    struct W {
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        std::function<int()> job;
        std::atomic<uint64_t> posted{0}, done{0};
        int rc = 0;
        std::string err;
        bool stop = false;
    };
    std::vector<W *> ws;
    static constexpr long kSpinUs = 1500;

    explicit DevWorkers(size_t n) {
        for (size_t i = 0; i < n; ++i) {
            W *w = new W();
            ws.push_back(w);
            w->th = std::thread([this, w]() { run(w); });
        }
    }
    ~DevWorkers() {
        for (W *w : ws) {
            { std::lock_guard<std::mutex> g(w->mu); w->stop = true; }
            w->cv.notify_one();
            w->th.join();
            delete w;
        }
    }
    void run(W *w) {
        uint64_t seen = 0;
        for (;;) {
            const auto t0 = std::chrono::steady_clock::now();
            unsigned spins = 0;
            while (w->posted.load(std::memory_order_acquire) == seen) {
                if ((++spins & 255u) == 0 &&
                    std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > kSpinUs) {
                    std::unique_lock<std::mutex> lk(w->mu);
                    w->cv.wait(lk, [&]() { return w->stop || w->posted.load(std::memory_order_acquire) != seen; });
                    if (w->stop) return;
                    break;
                }
                __builtin_ia32_pause();
            }
            seen = w->posted.load(std::memory_order_acquire);
            // a job that throws (std::bad_alloc out of a result vector's resize) must not take the process down with
            // std::terminate, nor leave wait() spinning on a worker that is gone: the error travels like any other
            try {
                w->rc = w->job();
                if (w->rc) w->err = g_err;
            } catch (const std::bad_alloc &) {
                w->rc = FZ_ENOMEM; w->err = "out of memory on a device worker thread";
            } catch (const std::exception &e) {
                w->rc = FZ_EDEVICE; w->err = std::string("exception on a device worker thread: ") + e.what();
            }
            w->done.store(seen, std::memory_order_release);
        }
    }
    void post(size_t i, std::function<int()> fn) {
        W *w = ws[i];
        // one job at a time per worker (the slot is overwritten below): callers wait for a job before they post the next; should
        // one ever not, the post waits here instead of corrupting the slot (rounds 4-5: an assert, i.e. abort() of the host process)
        while (w->done.load(std::memory_order_acquire) != w->posted.load(std::memory_order_relaxed)) std::this_thread::yield();
        w->job = std::move(fn);
        w->posted.fetch_add(1, std::memory_order_release);
        { std::lock_guard<std::mutex> g(w->mu); }
        w->cv.notify_one();
    }
    int wait(size_t i) {
        W *w = ws[i];
        const uint64_t want = w->posted.load(std::memory_order_relaxed);
        unsigned spins = 0;
        while (w->done.load(std::memory_order_acquire) != want) {
            if ((++spins & 1023u) == 0) std::this_thread::yield(); else __builtin_ia32_pause();
        }
        if (w->rc) g_err = w->err;
        return w->rc;
    }
};

// What collecting one shard of a multi-shard search leaves behind (one per shard, kept between searches).
struct ShardOut {
    std::vector<FzRec> recs;
    std::vector<uint64_t> hits;
    std::vector<fz_match> rows;                  // the shard's records in the reference's order (multi-shard searches)
    bool rerun = false;
    uint64_t nh = 0, nr = 0, bytes = 0;
    TimingRef tref{};                            // d == nullptr: the search was not timed
};

}  // namespace

struct fz_ctx {
    std::vector<DevState> devs;
    fz_stats_t stats{};
    // Candidate slots per list of the per-hit automaton kernel.  Small lists let every wave of the launch
    // be resident at once (256 slots: 8 KB of LDS per wave, 19 waves per CU; 1024: 7 per CU); a search
    // that overflows them re-runs with 4x the slots and the context remembers.
    uint32_t gen_cand_cap = 256;
    // The per-hit automaton runs as fz_gen_hit_kernel (a workgroup of 2 or 4 waves per hit).  A search in which a hit
    // outgrows a wave's share of the candidate list or its match buffer is run again with fz_lp_kernel (one wave per hit),
    // and so are the next gen_multi_skip searches of the context (1, 2, 4 .. 64 after consecutive failures; a success
    // resets the back-off): inputs that always fail (dense repeats) pay a wasted launch now and then, not every time.
    bool gen_multi = !sw().gen_legacy;
    uint32_t gen_multi_skip = 0, gen_multi_backoff = 0;
    // Single-shard searches in direct mode leave their records in the pinned staging buffer and only
    // publish a view of them (valid until the next search of this context): saves a 24 B x nr memcpy.
    const FzRec *view = nullptr;
    uint64_t view_n = 0;
    const FzGenRec *gen_view = nullptr;          // same for the per-hit automaton's records (pinned h_big)
    uint64_t gen_view_n = 0;
    const uint8_t *gen_rows_dev = nullptr;       // ... or the finished rows, ordered on the device (DevState::d_gen_rows)
    uint64_t gen_rows_n = 0;
    int gen_rows_device = 0;
    struct fz_stream *stream_inflight = nullptr;  // a file stream whose batch is on the device (other searches are refused)
    // fz_lev_ngrams_begin .. _end: up to two searches in flight, collected in launch order (pend[0] is the
    // oldest and owns the devices' current result slot, pend[1] their second slot)
    struct Pending {
        fz_seq *seq = nullptr;
        std::vector<uint8_t> pattern;
        uint32_t m = 0, k = 0;
        bool launched = false;                       // false: deferred until the older search has been collected
        uint32_t kind = FZ_MODE_LEV;                 // FZ_MODE_LEV / FZ_MODE_SUBS (result slots of lane 0) or FZ_MODE_GENERIC (lanes)
        uint32_t max_subs = 0, max_ins = 0, max_dels = 0;
        bool consolidated = false;                   // generic: deliver fz_generic_ngrams_consolidated's rows
        int lane = 0;                                // generic: which lane carries it
    } pend[2];
    int npend = 0;
    // Lanes: a second complete set of per-device state (stream, hit list, counters + records, ordering areas, staging).
    // A generic search in flight keeps its hit list and records on the device until it is collected, so the next one
    // needs buffers and a stream of its own: then its scan runs next to the older search's automaton kernel.
    std::vector<DevState> devs2;
    int lane = 0;                                // the lane the code below works on (0 except inside generic begin / end)
    // sequences still resident (fz_destroy frees what the caller did not release)
    std::vector<fz_seq *> live;
    // RCCL: number of ranks of the communicator this context joined (0: none) and whether its Levenshtein n-gram
    // searches are collective (every rank gets the merged global stream)
    bool any_found = false;                      // result of the last has_near_match_* (fz_*_any) search
    double rec_ms[4] = {0, 0, 0, 0};             // fz_debug_records_ms: the last fz_batch_upload_records
    double drv_ms[5] = {0, 0, 0, 0, 0};          // fz_debug_derive_ms: the last fz_batch_derive
    double fmt_ms[5] = {0, 0, 0, 0, 0};          // fz_debug_format_ms: the last fz_batch_format
    double ovl_ms[4] = {0, 0, 0, 0};             // fz_debug_overlap_ms: the last fz_batch_end_overlaps
    double cut_ms[4] = {0, 0, 0, 0};             // fz_debug_cuts_ms: the last fz_batch_score_cuts
    bool batch_call = false;                     // inside fz_batch_search: the one caller a batch handle is valid for (validate)
    // sharded searches: where every shard's (rank's) records end in the collected vector, and the shards in ascending
    // order of the index range they own (emit_matches orders shard by shard)
    std::vector<size_t> seg_ends;
    std::vector<uint32_t> seg_order;
    // hipEvent timing of the kernels (fz_stats: filter_ms / verify_ms / device_ms).  One event record is one more packet
    // in front of the kernel and two hipEventElapsedTime calls behind it: fz_set_timing(ctx, 0) drops them.
    bool timing = true;
    // The spans are read from the events only when somebody asks (fz_stats / fz_device_ms): a hipEventElapsedTime call
    // costs ~5 us of host time, two or three of them sat between the completion of every search and its result.  The
    // references die with the next launch of the context (whose enqueue re-records the events).
    std::vector<TimingRef> tref;
    int comm_world = 0;
    bool snapshot = false;
    bool comm_broken = false;                    // a collective ran into its deadline: the communicator is abandoned (no further
                                                 // collective is started, its streams and buffers are not waited for or freed)
    uint64_t gcap = 4096;                        // records per rank the all-gather carries (follows the counts, on all ranks alike)
    // fz_set_streams: 2 = the younger of two fused searches in flight scans on the other stream of its device, next to the
    // older one; 1 = behind it on the same stream.  fz_create sets the default (2 for a context of one device state).
    int streams = 1;
    // fz_set_scan_direction: 0 = every eligible scan launch starts where the shard's last one ended (alternating
    // directions), 1 = always forward, 2 = always reversed; and the reversed launches so far (fz_debug_scan_direction)
    int scan_dir = sw().scan_dir;
    std::atomic<uint64_t> rev_launches{0};
    double last_gather_ms = 0;                   // host time of the last search's exchange step (all-gather + D2H + parse)
    // multi-device contexts: one host thread per device (enqueue, wait, collect and order its shard), and what the
    // shards of the search being collected left (rows_ready: every shard's rows are ordered, emit_matches only merges)
    DevWorkers *workers = nullptr;
    std::vector<ShardOut> souts;
    bool rows_ready = false;
};

struct fz_seq {
    fz_ctx *ctx = nullptr;
    uint64_t n = 0;                              // global length
    std::vector<Shard> shards;
    // collective searches: the first index every rank of the communicator owns of THIS sequence (~0: nothing), exchanged
    // on the sequence's first collective search; the ranks' segments are merged in that order
    std::vector<uint64_t> rank_lo;
    // fz_batch_upload: n_seqs sequences packed back to back (fz_device.h: ragged segments).  ends = the host copy of the
    // cumulative end offsets (rows -> sequences).  The device tables (null for an empty batch): d_ends_base = the scanned
    // length table, n_seqs + 1 entries of which the first is 0, so the kernels' ends[] is d_ends_base + 1; d_first.
    bool is_batch = false;
    uint64_t n_seqs = 0;
    std::vector<uint64_t> ends;
    uint64_t *d_ends_base = nullptr;
    uint32_t *d_first = nullptr;
    uint64_t max_seq_len = 0;                    // the longest sequence (fz_batch_assign: local starts are 32-bit key fields)
    // fz_batch_upload_records, _fasta: the sequences' offsets in the text they were cut from stay on the device until
    // somebody asks (fz_batch_tables)
    uint64_t *d_src_starts = nullptr;
    // fz_batch_upload_fasta: the index rows, on the device until somebody asks (fz_batch_fasta_index)
    FzFaRow *d_fa_rows = nullptr;
    bool is_fasta = false;
};

namespace {
void comm_teardown(fz_ctx *ctx);
inline DevState &lane_dev(fz_ctx *ctx, int dev) { return ctx->lane ? ctx->devs2[dev] : ctx->devs[dev]; }

// fz_stats / fz_device_ms: the kernel spans of the search collected last, read from its events now.
void resolve_timing(fz_ctx *ctx) {
    for (const TimingRef &r : ctx->tref) {
        float f = 0, v = 0, t = 0;
        if (hipSetDevice(r.d->device) != hipSuccess) continue;
        if (r.f0 && hipEventElapsedTime(&f, r.f0, r.f1) != hipSuccess) f = 0;
        if (r.v0 && hipEventElapsedTime(&v, r.v0, r.v1) != hipSuccess) v = 0;
        if (r.t0 && hipEventElapsedTime(&t, r.t0, r.t1) != hipSuccess) t = 0;
        (void)hipGetLastError();
        r.d->last_filter_ms = f;
        ctx->stats.filter_ms = std::max<double>(ctx->stats.filter_ms, f);
        ctx->stats.verify_ms = std::max<double>(ctx->stats.verify_ms, v);
        ctx->stats.device_ms = std::max<double>(ctx->stats.device_ms, t);
    }
    ctx->tref.clear();
}
}

namespace {

// A device buffer that only grows: one that holds fewer than `cap` units is freed and allocated again with `bytes` bytes
// (its contents are lost; a buffer that a kernel in flight may still use is synchronised by the caller).
template <class T>
int grow_device(DevState &d, T *&ptr, uint64_t &have, uint64_t cap, uint64_t bytes) {
    if (have >= cap) return FZ_OK;
    HIP_TRY(hipSetDevice(d.device));
    if (ptr) { HIP_TRY(hipFree(ptr)); ptr = nullptr; have = 0; }
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ptr), (size_t)bytes));
    have = cap;
    return FZ_OK;
}

// The span between two recorded, completed events in ms; 0 (and no pending HIP error) if it cannot be read.
double span_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) ms = 0;
    (void)hipGetLastError();
    return (double)ms;
}

int ensure_hits(DevState &d, uint64_t cap) { return grow_device(d, d.d_hits, d.hit_cap, cap, cap * sizeof(uint64_t)); }

constexpr uint32_t kCandLdsMax = 4096;            // candidate slots per list that still live in LDS
constexpr uint32_t kCandMax = 1u << 18;           // ... and in the HBM fallback (4 MiB per workgroup)
constexpr unsigned kCandScratchGrid = 256;        // workgroups of a launch that uses the HBM lists

// LDS bytes and (if the lists do not fit LDS) the HBM scratch of one automaton launch.
int cand_lists(DevState &d, uint32_t cand_cap, size_t fixed_lds, size_t &lds, uint64_t &scratch) {
    if (fixed_lds > 150 * 1024) return fail(FZ_EUNSUPPORTED, "subsequence + window too long for the automaton kernel's LDS (%zu bytes)", fixed_lds);
    lds = fixed_lds + 2 * (size_t)cand_cap * sizeof(FzGCand);
    scratch = 0;
    const uint32_t lds_max = sw().cand_lds_max > 0 ? (uint32_t)sw().cand_lds_max : kCandLdsMax;   // (test knob: the HBM lists at small sizes)
    if (cand_cap <= lds_max && lds <= 160 * 1024) return FZ_OK;
    if (cand_cap > kCandMax) return fail(FZ_EUNSUPPORTED, "automaton candidate sets beyond %u entries", kCandMax);
    lds = fixed_lds;
    const uint64_t need = (uint64_t)kCandScratchGrid * 2 * cand_cap * sizeof(FzGCand);
    int rc = grow_device(d, d.d_cand, d.cand_bytes, need, need);
    if (rc) return rc;
    scratch = reinterpret_cast<uint64_t>(d.d_cand);
    return FZ_OK;
}

int ensure_big(DevState &d, uint64_t cap) {
    if (d.big_cap >= cap) return FZ_OK;
    HIP_TRY(hipSetDevice(d.device));
    if (d.h_big) { HIP_TRY(hipStreamSynchronize(d.stream)); HIP_TRY(hipHostFree(d.h_big)); d.h_big = nullptr; d.big_cap = 0; }
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&d.h_big), cap * sizeof(FzRec), hipHostMallocMapped));
    d.big_cap = cap;
    return FZ_OK;
}

// Ordering area and row buffer of the device-ordered generic search (rows follow the record capacity).
int ensure_gen_rows(DevState &d) {
    HIP_TRY(hipSetDevice(d.device));
    if (!d.d_gen_order) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d.d_gen_order), (size_t)FZ_GEN_ORDER_MAX * 12));
    return grow_device(d, d.d_gen_rows, d.gen_rows_cap, d.rec_cap, d.rec_cap * sizeof(FzOutRow));
}

// Snapshot buffers of a communicator's device state: at least `cap` records each; contents are kept (a snapshot
// that is waiting for its all-gather survives the growth).
int ensure_send(DevState &d, uint64_t cap) {
    if (d.send_cap >= cap && d.slots[0].d_send) return FZ_OK;
    HIP_TRY(hipSetDevice(d.device));
    for (ResultSlot &s : d.slots) {
        uint8_t *nb = nullptr;
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&nb), kHeaderBytes + cap * sizeof(FzRec)));
        if (s.d_send) {
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipMemcpy(nb, s.d_send, kHeaderBytes + d.send_cap * sizeof(FzRec), hipMemcpyDeviceToDevice));
            HIP_TRY(hipFree(s.d_send));
        } else {
            HIP_TRY(hipMemset(nb, 0, kHeaderBytes));
        }
        s.d_send = nb;
    }
    d.send_cap = cap;
    return FZ_OK;
}

int ensure_recs(DevState &d, uint64_t cap) {
    if (d.rec_cap >= cap) return FZ_OK;
    int rc = grow_device(d, d.d_out, d.rec_cap, cap, kHeaderBytes + cap * sizeof(FzRec));
    if (rc) return rc;
    d.header_zeroed = false;
    return FZ_OK;
}

uint32_t load_le32(const uint8_t *p, uint32_t avail) {
    uint32_t v = 0;
    for (uint32_t i = 0; i < 4 && i < avail; ++i) v |= (uint32_t)p[i] << (8 * i);
    return v;
}

// Describes one whole search as a list of n-gram blocks.
struct BlockPlan {
    uint32_t L = 0;
    std::vector<uint32_t> s;       // ngram_start per block (the accepted hit range follows from it: fz_block_range)
    uint64_t abs_lo = 0, abs_hi = ~0ull;   // absolute index range (exact search with start / end index)
};

using LpKernel = void (*)(const uint8_t *, const FzScanArgs, const uint64_t *, uint64_t, FzGenRec *, unsigned long long *);

LpKernel lp_kernel(uint32_t kind, bool hbm_lists) {
    switch (kind) {
    case FZ_LP_GENERIC_HIT: return hbm_lists ? fz_lp_kernel<FZ_LP_GENERIC_HIT, true> : fz_lp_kernel<FZ_LP_GENERIC_HIT, false>;
    case FZ_LP_GENERIC_SEQ: return hbm_lists ? fz_lp_kernel<FZ_LP_GENERIC_SEQ, true> : fz_lp_kernel<FZ_LP_GENERIC_SEQ, false>;
    default: return hbm_lists ? fz_lp_kernel<FZ_LP_LEV_SEQ, true> : fz_lp_kernel<FZ_LP_LEV_SEQ, false>;
    }
}

using ScanKernel = void (*)(const uint8_t *, const FzScanArgs, uint64_t, uint64_t *, FzRec *, unsigned long long *);

template <bool FUSED, bool SEG, bool SA>
ScanKernel scan_kernel_f(int nwin, int dh) {
    if (nwin == 1) return fz_scan_kernel<1, 0, FUSED, SEG, SA>;
    switch (dh) {
        case 2: return fz_scan_kernel<2, 2, FUSED, SEG, SA>;
        case 3: return fz_scan_kernel<2, 3, FUSED, SEG, SA>;
        case 4: return fz_scan_kernel<2, 4, FUSED, SEG, SA>;
        default: return fz_scan_kernel<2, 5, FUSED, SEG, SA>;
    }
}

template <bool FUSED, bool SEG>
ScanKernel scan_kernel_s(int nwin, int dh, bool sa) {
    return sa ? scan_kernel_f<FUSED, SEG, true>(nwin, dh) : scan_kernel_f<FUSED, SEG, false>(nwin, dh);
}

// The segmented variants (file API) only exist where a segment changes the outcome: Levenshtein /
// generic clamps.  Exact and substitutions-only windows fit exactly one chunk (the host assigns it).
// sa: the launch's blocks are told apart by hash bits 2..6 (slot address = one v_and).
// The fused lane-per-cell form (Levenshtein budgets 5 .. 15 of in-memory searches, fz_flush_wf): GW = 16 or 32 lanes per candidate.
template <bool SA, int GW>
ScanKernel scan_kernel_wf(int nwin, int dh) {
    if (nwin == 1) return fz_scan_kernel<1, 0, true, false, SA, GW>;
    switch (dh) {
        case 2: return fz_scan_kernel<2, 2, true, false, SA, GW>;
        case 3: return fz_scan_kernel<2, 3, true, false, SA, GW>;
        case 4: return fz_scan_kernel<2, 4, true, false, SA, GW>;
        default: return fz_scan_kernel<2, 5, true, false, SA, GW>;
    }
}

// wf_gw: 0 = register band / Hamming count, 1 / 2 = bit-vector columns on one / two 64-bit words, 4 = on one 32-bit word,
// 3 = Hamming count under the bit-vector forms' queue discipline (dense candidates), 16 / 32 = lanes per candidate
ScanKernel scan_kernel(int nwin, int dh, bool fused, bool seg, bool sa, int wf_gw = 0) {
#ifdef FZ_LAB_ONLY      // lab builds (benchmarks/lab_build.sh): only the instances of the headline and exact-search workloads
    if (wf_gw == 1 && nwin == 2 && dh == 3 && fused && !seg) return sa ? fz_scan_kernel<2, 3, true, false, true, 1> : fz_scan_kernel<2, 3, true, false, false, 1>;
    if (wf_gw == 3 && nwin == 2 && dh == 3 && fused && !seg) return sa ? fz_scan_kernel<2, 3, true, false, true, 3> : fz_scan_kernel<2, 3, true, false, false, 3>;
    if (wf_gw == 2 && nwin == 2 && dh == 3 && fused && !seg) return sa ? fz_scan_kernel<2, 3, true, false, true, 2> : fz_scan_kernel<2, 3, true, false, false, 2>;
    if (wf_gw == 4 && nwin == 2 && dh == 3 && fused && !seg) return sa ? fz_scan_kernel<2, 3, true, false, true, 4> : fz_scan_kernel<2, 3, true, false, false, 4>;
    if (wf_gw) return nullptr;
    if (nwin == 2 && dh == 3 && fused && !seg) return sa ? fz_scan_kernel<2, 3, true, false, true> : fz_scan_kernel<2, 3, true, false, false>;
    if (nwin == 2 && dh == 5 && !fused && !seg) return sa ? fz_scan_kernel<2, 5, false, false, true> : fz_scan_kernel<2, 5, false, false, false>;
    return nullptr;
#else
    if (wf_gw == 1) return seg ? nullptr : (sa ? scan_kernel_wf<true, 1>(nwin, dh) : scan_kernel_wf<false, 1>(nwin, dh));
    if (wf_gw == 2) return seg ? nullptr : (sa ? scan_kernel_wf<true, 2>(nwin, dh) : scan_kernel_wf<false, 2>(nwin, dh));
    if (wf_gw == 4) return seg ? nullptr : (sa ? scan_kernel_wf<true, 4>(nwin, dh) : scan_kernel_wf<false, 4>(nwin, dh));
    if (wf_gw == 3) return seg ? nullptr : (sa ? scan_kernel_wf<true, 3>(nwin, dh) : scan_kernel_wf<false, 3>(nwin, dh));
    if (wf_gw == 16) return seg ? nullptr : (sa ? scan_kernel_wf<true, 16>(nwin, dh) : scan_kernel_wf<false, 16>(nwin, dh));
    if (wf_gw == 32) return seg ? nullptr : (sa ? scan_kernel_wf<true, 32>(nwin, dh) : scan_kernel_wf<false, 32>(nwin, dh));
    if (seg) return fused ? scan_kernel_s<true, true>(nwin, dh, sa) : scan_kernel_s<false, true>(nwin, dh, sa);
    return fused ? scan_kernel_s<true, false>(nwin, dh, sa) : scan_kernel_s<false, false>(nwin, dh, sa);
#endif
}

// The lean instances (fz_kernels.h: fz_lean_scan_kernel): the in-memory register-band / Hamming-count form without the
// equal-n-gram slot sets and without the bands for k = 3, 4.
template <bool SA>
ScanKernel lean_scan_kernel_f(int nwin, int dh) {
#ifdef FZ_LAB_ONLY
    return nwin == 2 && dh == 3 ? fz_lean_scan_kernel<2, 3, SA> : nullptr;
#else
    if (nwin == 1) return fz_lean_scan_kernel<1, 0, SA>;
    switch (dh) {
        case 2: return fz_lean_scan_kernel<2, 2, SA>;
        case 3: return fz_lean_scan_kernel<2, 3, SA>;
        case 4: return fz_lean_scan_kernel<2, 4, SA>;
        default: return fz_lean_scan_kernel<2, 5, SA>;
    }
#endif
}

ScanKernel lean_scan_kernel(int nwin, int dh, bool sa) { return sa ? lean_scan_kernel_f<true>(nwin, dh) : lean_scan_kernel_f<false>(nwin, dh); }

// Lean or full, for one launch of a scan: lean where nothing the full instance carries on top can run — the register-band /
// Hamming-count form (wf_gw = 0) of a fused in-memory search over one sequence, no two blocks of the launch with the same
// hash, and Levenshtein with a budget of at most 2 or substitutions only.  Everything else — equal n-grams, k = 3 and 4 on
// the band when the switches keep the bit-vector forms away — takes the full instance.  A function of the search's
// arguments and the switches, as plan_scan and choose_launch_blocks are.
bool scan_is_lean(uint32_t mode, uint32_t k, const FzScanArgs &fa, int wf_gw, bool seg, bool ragged) {
    if (!fa.fused || seg || ragged || wf_gw != 0 || (fa.flags & FZ_FLAG_DUP_HASHES)) return false;
    return mode == FZ_MODE_SUBS || (mode == FZ_MODE_LEV && k <= 2);
}

// The ragged instances (fz_batch_search: a batch of sequences packed back to back): every form of the in-memory search.
// The register-band / Hamming-count / hit-emitting forms come with and without the one-v_and slot address (sa); the
// bit-vector and lane-per-cell forms only in the general form, which serves every slot shift.
template <bool FUSED, bool SA, int WFG>
ScanKernel batch_scan_kernel_f(int nwin, int dh) {
    if (nwin == 1) return fz_batch_scan_kernel<1, 0, FUSED, SA, WFG>;
    switch (dh) {
        case 2: return fz_batch_scan_kernel<2, 2, FUSED, SA, WFG>;
        case 3: return fz_batch_scan_kernel<2, 3, FUSED, SA, WFG>;
        case 4: return fz_batch_scan_kernel<2, 4, FUSED, SA, WFG>;
        default: return fz_batch_scan_kernel<2, 5, FUSED, SA, WFG>;
    }
}

ScanKernel batch_scan_kernel(int nwin, int dh, bool fused, bool sa, int wf_gw) {
    switch (wf_gw) {
        case 1: return batch_scan_kernel_f<true, false, 1>(nwin, dh);
        case 2: return batch_scan_kernel_f<true, false, 2>(nwin, dh);
        case 3: return batch_scan_kernel_f<true, false, 3>(nwin, dh);
        case 4: return batch_scan_kernel_f<true, false, 4>(nwin, dh);
        case 16: return batch_scan_kernel_f<true, false, 16>(nwin, dh);
        case 32: return batch_scan_kernel_f<true, false, 32>(nwin, dh);
        default: break;
    }
    if (fused) return sa ? batch_scan_kernel_f<true, true, 0>(nwin, dh) : batch_scan_kernel_f<true, false, 0>(nwin, dh);
    return sa ? batch_scan_kernel_f<false, true, 0>(nwin, dh) : batch_scan_kernel_f<false, false, 0>(nwin, dh);
}

// Odd multipliers tried for the window hash (24-bit ones serve v_mad_u32_u24).  One search needs a
// multiplier under which its (at most 16 per launch) distinct block hashes fall into distinct slots of
// the 32-slot table: a random one works with probability 0.91 for 3 blocks, 0.39 for 8.
const uint32_t kHashMultipliers[] = {0x9E3779u, 0x85EBCBu, 0xC2B2AFu, 0x27D4EBu, 0x165667u, 0xD3A264u | 1u, 0xFD7047u, 0xB55A4Fu,
                                     0x7FEB35u, 0x846CA7u, 0x9E6C63u, 0x3243F7u, 0x517CC1u, 0xB7E151u, 0x6A09E7u, 0xBB67AFu,
                                     // (round 6: launches carry up to 16 blocks — more tries for the rarer perfect placements)
                                     0x3C6EF3u, 0xA54FF5u, 0x510E53u, 0x9B0569u, 0x1F83D9u, 0x5BE0CDu, 0xCA62C1u, 0x8F1BBDu,
                                     0x6ED9EBu, 0x5A8279u, 0xC3D2E1u, 0x10325Fu, 0x98BADDu, 0xEFCDABu, 0x674523u, 0x2B7E15u};

// Window geometry of the filter's hash for n-gram length L (see fz_hash_windows / fz_hash_short).
struct HashGeom {
    int nwin;            // 1: L <= 4 (masked dword * K);  2: dword + 24 bits at offset dh
    int dh;
    uint32_t mask1;
    explicit HashGeom(uint32_t L)
        : nwin(L <= 4 ? 1 : 2), dh(L <= 4 ? 0 : (int)std::min<uint32_t>(L, 8) - 3),
          mask1(L >= 4 ? 0xffffffffu : ((1u << (8 * L)) - 1u)) {}
    uint32_t hash(const uint8_t *ng, uint32_t L, uint32_t k) const {
        const uint32_t a1 = load_le32(ng, L) & mask1;
        return nwin == 2 ? fz_hash_windows(a1, load_le32(ng + dh, 3), k) : fz_hash_short(a1, k);
    }
};

// Blocks [g0, g0 + n) of one scan launch, the hash multiplier and the slot bits: the longest run of
// blocks (at most 16) whose distinct hashes land in distinct slots of the 32-slot table under some
// (multiplier, shift).  One block always fits; equal n-grams (equal hashes) share a slot.
// h = yh * K + x mixes x only through the addition: which five bits tell the blocks apart depends on
// where their bytes differ, so the slot bits are a per-launch choice as well.
uint32_t choose_launch_blocks(const uint8_t *p, const uint32_t *starts, uint32_t g0, uint32_t G, uint32_t L,
                              uint32_t &hash_k, uint32_t &lut_shift) {
    const HashGeom hg(L);
    // FZ_MAX_BLOCKS=n (test knob): at most n blocks per launch, to exercise the multi-launch path
    const uint32_t max_blocks = sw().max_blocks > 0 ? std::min<uint32_t>((uint32_t)sw().max_blocks, FZ_MAX_BLOCKS_PER_LAUNCH)
                                                             : FZ_MAX_BLOCKS_PER_LAUNCH;
    const bool no_sa = sw().no_slot_and;                               // test knob: never use the low-bits form
    const uint32_t want = std::min<uint32_t>(max_blocks, G - g0);
    uint32_t nblk = 0;
    // Pass 0: hash bits 2..6 as they are (lut_shift == 2: the kernel forms the slot address with one v_and; those
    // bits only see window bytes 0 and DH) — taken only if it fits every block this launch could carry.
    // Pass 1: any aligned group of five hash bits.
    for (int pass = no_sa ? 1 : 0; pass < 2; ++pass) {
        for (uint32_t cand : kHashMultipliers) {
            const uint32_t kk = hg.nwin == 2 ? cand : (cand * 0x9E3779B1u) | 1u;
            uint32_t hb[FZ_MAX_BLOCKS_PER_LAUNCH];
            uint32_t nb = 0;
            for (; nb < want; ++nb) hb[nb] = hg.hash(p + starts[g0 + nb], L, kk);
            for (int shift = pass == 0 ? 2 : 32 - FZ_LUT_BITS; shift >= 2; shift -= FZ_LUT_BITS) {
                uint32_t slot_hash[FZ_LUT_SLOTS];
                bool used[FZ_LUT_SLOTS] = {false};
                uint32_t fit = 0;
                for (; fit < nb; ++fit) {
                    const uint32_t slot = (hb[fit] >> shift) & (FZ_LUT_SLOTS - 1u);
                    if (used[slot] && slot_hash[slot] != hb[fit]) break;
                    used[slot] = true;
                    slot_hash[slot] = hb[fit];
                }
                if (fit > nblk && (pass == 1 || fit == want)) { nblk = fit; hash_k = kk; lut_shift = (uint32_t)shift; }
            }
            if (nblk == want) break;
        }
        if (nblk == want) break;
    }
    return nblk;
}

// a connected set of matches: its hull [h0, h1) and its best match (fz_consolidate, fz_generic_ngrams_consolidated)
struct Hull { int64_t h0, h1; fz_match best; };
int consolidate_hulls(std::vector<Hull> &hulls, fz_match **out, uint64_t *n_out);

int emit_generic(fz_ctx *ctx, fz_seq *seq, const std::vector<FzGenRec> &recs_vec, uint32_t L, uint32_t k, fz_match **out,
                 uint64_t *n, uint32_t **seg_out);

struct Search {
    uint32_t mode = 0, m = 0, k = 0;
    uint32_t max_subs = 0, max_ins = 0, max_dels = 0;      // generic search only
    const uint8_t *p = nullptr;
    BlockPlan plan;
    bool collective = false;       // the context joined a communicator: every rank gets the merged stream of all ranks
    bool any = false;              // has_near_match_*: only whether a record exists
    bool fold = false;             // generic search: the device folds every hit's matches into (hull, best match) pairs
    // has_near_match_* on a long single-shard sequence: the scan of THIS call covers the buffer bytes [part_lo, part_hi) only
    // (multiples of the tile size; hits are owned by the tile their index lies in, windows reach wherever they must)
    uint64_t part_lo = 0, part_hi = ~0ull;
};

// dynamic LDS per scan workgroup when verification is fused
constexpr uint32_t kFusedLdsBudget = 64u * 1024u;

// One kernel launch.  Its start / stop events (either may be null) ride on the kernel's own dispatch packet when there are
// any: no event packets of their own around it.
template <typename... KArgs, typename... Args>
void launch(void (*kernel)(KArgs...), dim3 grid, dim3 block, uint32_t lds, hipStream_t st, hipEvent_t ev_start,
            hipEvent_t ev_stop, Args... args) {
    if (ev_start || ev_stop) hipExtLaunchKernelGGL(kernel, grid, block, lds, st, ev_start, ev_stop, 0u, args...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
}

// Fields of FzScanArgs that every kernel of a search shares.
void fill_common_args(FzScanArgs &fa, const Shard &sh, const Search &q) {
    memset(&fa, 0, sizeof fa);
    fa.geom = sh.geom;
    fa.mode = q.mode;
    fa.m = q.m;
    fa.k = q.k;
    fa.L = q.plan.L;
    fa.max_subs = q.max_subs; fa.max_ins = q.max_ins; fa.max_dels = q.max_dels;
    fa.abs_lo = q.plan.abs_lo;
    fa.abs_hi = q.plan.abs_hi;
    if (q.m <= FZ_MAX_M) memcpy(fa.pat, q.p, q.m);
}


// The pattern in HBM, for kernels that do not (or cannot) take it from the kernel-argument block.  The copy is
// ordered on the device's stream like the kernels that read it (searches of one context run one after the other
// on that stream, so two searches in flight can share the buffer).
int stage_pattern(DevState &d, FzScanArgs &fa, const uint8_t *p, uint32_t m, bool force = false) {
    fa.pat_g = 0;
    if (m <= FZ_MAX_M && !force) return FZ_OK;
    HIP_TRY(hipSetDevice(d.device));
    if (d.pat_cap < m) {
        HIP_TRY(hipStreamSynchronize(d.stream));
        const uint64_t cap = std::max<uint64_t>(4096, (uint64_t)m * 2);
        int rc = grow_device(d, d.d_pat, d.pat_cap, cap, cap);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(d.d_pat, p, m, hipMemcpyHostToDevice, d.stream));
    fa.pat_g = reinterpret_cast<uint64_t>(d.d_pat);
    return FZ_OK;
}

// Lanes per candidate of the lane-per-cell verification: the 2k + 1 band cells of a row must fit.
int wavefront_group(uint32_t k) { return 2 * k + 1 <= 16 ? 16 : 2 * k + 1 <= 32 ? 32 : 64; }

// Which stand-alone verification a search takes when it is not fused into the scan: lane-per-cell with LDS windows
// (Levenshtein budgets 5 .. 31), lane-per-candidate with an LDS score ring (everything else that fits LDS), or —
// patterns beyond the argument block, budgets beyond FZ_MAX_K, windows / rings beyond LDS — one wave per hit straight
// from HBM (fz_verify_big_kernel).
struct VerifyPlan {
    bool want_wf = false, big = false;
    int gw = 16;
    size_t wf_lds = 0, ring_lds = 0;
    unsigned waves = 4;
};

VerifyPlan plan_verify(const Search &q) {
    const bool force_big = sw().force_big_verify;                               // test knob: every stand-alone verification by fz_verify_big_kernel
    VerifyPlan v;
    const uint32_t mpad = (q.m + 15u) & ~15u;
    const uint32_t win_dwords = (q.m + 2 * q.k + 6) / 4 + 1;
    const uint32_t band_w = q.mode == FZ_MODE_LEV ? 2 * q.k + 2 : 0;
    v.gw = wavefront_group(q.k);
    const uint32_t wf_per_wave = (64u / v.gw) * (win_dwords * 4u + 16u);       // one window per hit (at most 64 / gw hits per wave)
    v.wf_lds = 16 + mpad + 16 + 16 * (size_t)wf_per_wave;                       // 16 waves per workgroup
    while (v.waves > 1 && mpad + v.waves * (size_t)fz_wave_lds_bytes(win_dwords, band_w, 64, false) > 64 * 1024) v.waves >>= 1;
    v.ring_lds = mpad + (size_t)v.waves * fz_wave_lds_bytes(win_dwords, band_w, 64, false);
    v.want_wf = q.mode == FZ_MODE_LEV && q.k >= 5 && q.k <= 31;
    v.big = force_big || q.m > FZ_MAX_M || q.k > FZ_MAX_K || (v.want_wf ? v.wf_lds > 64 * 1024 : v.ring_lds > 160 * 1024);
    return v;
}

// The regions of a scan grid (FzScanArgs.reg_*; nreg = 0: every workgroup strides over all tiles).  `steps` groups of
// the last `t_per_cu x n_cus` workgroups take shares shrinking to `fmin` of a full one.
void plan_scan_regions(FzScanArgs &fa, uint64_t ntiles, uint64_t grid, uint32_t n_cus, int steps, double fmin, int t_per_cu) {
    fa.nreg = 0;
    steps = std::min(steps, FZ_MAX_REGIONS - 1);
    fmin = std::min(1.0, std::max(0.02, fmin));
    const uint64_t Gw = grid, T = (uint64_t)n_cus * (uint64_t)std::max(1, t_per_cu);
    if (steps <= 0 || (uint64_t)steps > T || Gw < 2 * T || ntiles < 4 * Gw) return;
    const uint64_t per = T / steps;                            // workgroups per taper group (the last group takes the rest)
    double weight = (double)(Gw - T);
    std::vector<double> f(steps);
    std::vector<uint64_t> nw(steps);
    for (int j = 0; j < steps; ++j) {
        f[j] = 1.0 - (1.0 - fmin) * (j + 1) / steps;
        nw[j] = j + 1 < steps ? per : T - per * (steps - 1);
        weight += f[j] * (double)nw[j];
    }
    const double share = (double)ntiles / weight;              // tiles of a full workgroup
    uint64_t at = 0, wg = 0;
    auto add = [&](uint64_t nwg, uint64_t tiles) {
        fa.reg_wg0[fa.nreg] = (uint32_t)wg; fa.reg_nwg[fa.nreg] = (uint32_t)nwg;
        fa.reg_tile0[fa.nreg] = at; fa.reg_end[fa.nreg] = at + tiles;
        ++fa.nreg; wg += nwg; at += tiles;
    };
    add(Gw - T, std::min<uint64_t>(ntiles, (uint64_t)(share * (double)(Gw - T) + 0.5)));
    for (int j = 0; j < steps; ++j) {
        const uint64_t left = ntiles - at;
        add(nw[j], j + 1 < steps ? std::min<uint64_t>(left, (uint64_t)(share * f[j] * (double)nw[j] + 0.5)) : left);
    }
    // the queue codes carry a bounded per-workgroup tile iteration
    for (uint32_t r = 0; r < fa.nreg; ++r)
        if ((fa.reg_end[r] - fa.reg_tile0[r] + fa.reg_nwg[r] - 1) / fa.reg_nwg[r] >= FZ_TITER_MAX) { fa.nreg = 0; break; }
}

// ... with the process-wide settings (FZ_TAPER_STEPS, default 4; FZ_TAPER_MIN, default 0.25; FZ_TAPER_WG_PER_CU, default 7 =
// the workgroups of this kernel that are resident per CU).
void plan_scan_regions(FzScanArgs &fa, uint64_t ntiles, uint64_t grid, uint32_t n_cus) {
    const int steps = sw().taper_steps;
    const double fmin = sw().taper_min;
    const int t_per_cu = sw().taper_wg_per_cu;
    plan_scan_regions(fa, ntiles, grid, n_cus, steps, fmin, t_per_cu);
}

// FZ_SCAN_ROUNDS=1, the plan of a scan next to its predecessor: {first resident round | middle | last resident round}.  With
// nreg = 0 every workgroup strides over the whole buffer, so what a launch reads last is spread over all of it; here the
// first and the last `n_cus x taper_wg_per_cu` workgroups stride over a range of their own at the start / the end of the
// buffer (one workgroup's share each, as before), which the chip then sweeps in address order, one resident front (~28 MiB)
// at a time — what a mirrored successor re-reads first is what this launch read last.  Grids below two fronts keep nreg = 0.
void plan_scan_rounds(FzScanArgs &fa, uint64_t ntiles, uint64_t grid, uint32_t n_cus) {
    fa.nreg = 0;
    const uint64_t W = (uint64_t)n_cus * (uint64_t)std::max(1, sw().taper_wg_per_cu);
    if (grid < 2 * W || ntiles < 4 * grid) return;
    const uint64_t edge = ntiles * W / grid, mid = grid - 2 * W;
    uint64_t at = 0, wg = 0;
    auto add = [&](uint64_t nwg, uint64_t tiles) {
        if (!nwg) return;
        fa.reg_wg0[fa.nreg] = (uint32_t)wg; fa.reg_nwg[fa.nreg] = (uint32_t)nwg;
        fa.reg_tile0[fa.nreg] = at; fa.reg_end[fa.nreg] = at + tiles;
        ++fa.nreg; wg += nwg; at += tiles;
    };
    add(W, mid ? edge : ntiles - edge);
    add(mid, ntiles - 2 * edge);
    add(W, edge);
    for (uint32_t r = 0; r < fa.nreg; ++r)
        if ((fa.reg_end[r] - fa.reg_tile0[r] + fa.reg_nwg[r] - 1) / fa.reg_nwg[r] >= FZ_TITER_MAX) { fa.nreg = 0; break; }
}

// What one scan of a shard runs: the grid, the verification form and the sizes that go with them.  The shape fields of
// FzScanArgs (regions, fused, vlanes, qcap, win_pieces, win_dwords, band_w) are written into the scan's arguments.
struct ScanPlan {
    uint64_t ntiles = 0;         // tiles this call scans
    uint32_t grid = 1;           // workgroups of every scan launch
    int wfg = 0;                 // the scan kernel's WFG argument (scan_kernel: wf_gw)
    uint32_t form = FZ_FORM_NONE;   // fz_stats' verify_form
    uint32_t lds = 0;            // dynamic LDS of a scan workgroup
    VerifyPlan vp;               // the stand-alone verification (with_verify and not fused)
    bool overlapped = false;     // the launch runs next to the scan of the search in flight before it (enqueue_shard)
    bool partial = false;        // the call scans a piece of the buffer (has_near_match_* in growing pieces)
};

// Everything that decides what a scan of the shard with geometry `geom` runs: a function of the search, the geometry, the
// device's CU count, the switches and `shares_chip` (another search of the context is in flight on the device and this one
// writes its records straight to the host), no device state.  A fused in-memory scan that shares the chip is planned as
// one that runs next to its predecessor (sp.overlapped); every other plan is the same with or without `shares_chip`.
ScanPlan plan_scan(const Search &q, const FzGeom &geom, uint32_t n_cus, bool with_verify, bool shares_chip, FzScanArgs &fa) {
    ScanPlan sp;
    const uint32_t L = q.plan.L;
    const uint32_t G = (uint32_t)q.plan.s.size();
    const bool in_memory = geom.seg_stride == 0;
    const uint64_t ntiles_all = (geom.buf_len + FZ_TILE_BYTES - 1) / FZ_TILE_BYTES;
    const uint64_t tile_lo = std::min<uint64_t>(ntiles_all, q.part_lo / FZ_TILE_BYTES);
    const uint64_t tile_hi = q.part_hi == ~0ull ? ntiles_all : std::min<uint64_t>(ntiles_all, (q.part_hi + FZ_TILE_BYTES - 1) / FZ_TILE_BYTES);
    const bool partial = sp.partial = tile_lo != 0 || tile_hi != ntiles_all;
    const uint64_t ntiles = sp.ntiles = tile_hi > tile_lo ? tile_hi - tile_lo : 0;
    const bool force_big = sw().force_big_verify;
    sp.vp = plan_verify(q);
    const VerifyPlan &vp = sp.vp;
    fa.band_w = q.mode == FZ_MODE_LEV ? 2 * q.k + 2 : 0;
    fa.win_dwords = (q.m + 2 * q.k + 6) / 4 + 1;
    const uint32_t mpad = (q.m + 15u) & ~15u;
    // Lanes that verify at once: all 64 while the staged windows stay small; fewer for long patterns
    // so that the scan keeps ~8 workgroups per CU resident (measured at m = 64, k = 5 on 1 GiB of text:
    // 64 lanes -> 31.6 KB LDS, 5 workgroups/CU, scan 0.540 ms; candidates are rare there anyway).
    constexpr uint32_t target = 18u * 1024u;
    fa.vlanes = 64;
    uint32_t fused_lds;
    if (in_memory) {
        // in-memory search: the windows of queued candidates are prefetched by LDS-DMA, 16-byte pieces, one slot
        // per queue entry (fz_prefetch_windows); the queue shrinks for long patterns (a tile that outgrows it is
        // re-scanned by enumeration, 64 entries at a time: 64 is the floor)
        fa.win_pieces = (q.m + 2 * q.k + 3 + 15) / 16;           // window <= m + 2k bytes + 3 of dword alignment
        fa.qcap = 128;
        while (fa.qcap > 64 && mpad + FZ_TABLE_BYTES + FZ_WAVES_PER_BLOCK * fz_wave_lds_pref_bytes(fa.qcap, fa.win_pieces) > target + 4096)
            fa.qcap >>= 1;
        fused_lds = mpad + FZ_TABLE_BYTES + FZ_WAVES_PER_BLOCK * fz_wave_lds_pref_bytes(fa.qcap, fa.win_pieces);
        if (fa.win_pieces * 16u + 16u > FZ_PAD_BACK) fused_lds = ~0u;   // the last pieces may lie past the sequence: inside the padding only
    } else {
        while (fa.vlanes > 16 && mpad + FZ_TABLE_BYTES + FZ_WAVES_PER_BLOCK * fz_wave_lds_bytes(fa.win_dwords, fa.band_w, fa.vlanes, true) > target)
            fa.vlanes >>= 1;
        fused_lds = mpad + FZ_TABLE_BYTES + FZ_WAVES_PER_BLOCK * fz_wave_lds_bytes(fa.win_dwords, fa.band_w, fa.vlanes, true);
    }
    // k > 4 (register band too wide for the scan kernel's VGPR budget) -> lane-per-cell: inside the scan as well while 16
    // or 32 lanes hold the band (budgets 5 .. 15: the candidates of a wave's queue, four or two at a time), in a kernel of
    // its own beyond that
    fa.fused = (with_verify && !force_big && q.m <= FZ_MAX_M && q.k <= FZ_MAX_K && fused_lds <= kFusedLdsBudget &&
                (q.mode != FZ_MODE_LEV || q.k <= 4)) ? 1u : 0u;
    // Levenshtein budgets from FZ_BITS_MIN_K on, patterns up to 128 characters, in-memory: bit-vector columns, one candidate
    // per lane, inside the scan (fz_verify_lev_bits) — a column costs the same whatever the budget, so neither the band's
    // width nor the candidates' density decides the form.  The queue takes what LDS allows (full passes: fz_bits_flush).
    int bits_nw = 0;
    // Candidates a wave is expected to find in one tile (4 KiB of offsets per wave) if the sequence is uniform over the
    // symbols the PATTERN uses — G blocks of L characters over sigma symbols: 4096 G / sigma^L (DNA, m = 54, k = 8: 9;
    // m = 20, k = 4: 80; text patterns: next to nothing).  A function of the search's arguments, not of earlier calls; an
    // estimate that is off costs time, never rows.
    double per_tile = 0;
    {
        bool seen[256] = {false};
        uint32_t sigma = 0;
        for (uint32_t i = 0; i < q.m; ++i)
            if (!seen[q.p[i]]) { seen[q.p[i]] = true; ++sigma; }
        per_tile = 4096.0 * std::min<uint32_t>(G, FZ_MAX_BLOCKS_PER_LAUNCH);
        for (uint32_t i = 0; i < L && per_tile > 0.01; ++i) per_tile /= (double)std::max(2u, sigma);
    }
    // Which budgets: from FZ_BITS_MIN_K (3) on always — at k = 3 on DNA it is 20 % ahead of the register band, at k >= 5 it
    // replaces the lane-per-cell forms; below that only where the expected density is beyond what the register-band form's
    // queue discipline takes (more than ~16 candidates per tile and wave: short DNA patterns), the headline workload
    // (k = 2, 3 per tile) keeps the band.
    const bool bits_budget = q.k >= (uint32_t)sw().bits_min_k || per_tile > 16.0;
    // fz_verify_lev_bits packs its running minimum as (score << 8) | columns_left: windows of at most 255 columns.  The gate's
    // whole-piece bound win_pieces * 16 + 16 <= FZ_PAD_BACK (with m <= 128) keeps every window at m + 2k + 3 <= 240 columns.
    static_assert(FZ_PAD_BACK - 16 <= 255, "fz_verify_lev_bits: window columns in 8 bits");
    if (q.mode == FZ_MODE_LEV && with_verify && !force_big && !sw().no_bits && in_memory && bits_budget &&
        q.m <= FZ_BITS_MAX_M(2) && q.k <= FZ_MAX_K && fa.win_pieces * 16u + 16u <= FZ_PAD_BACK) {
        bits_nw = q.m <= FZ_BITS_MAX_M(4) ? 4 : q.m <= FZ_BITS_MAX_M(1) ? 1 : 2;      // 32-, 64-, 128-bit columns
        // (26 KB: six workgroups per CU.  Measured on 1 GiB of DNA, m = 54, k = 8, 2.4e6 candidates: 64 / 96 / 128 / 160 entries
        //  per wave = 26 / 37 / 47 / 58 KB -> 0.463 / 0.517 / 0.656 / 0.830 ms: fuller passes do not pay for the lost waves)
        constexpr uint32_t budget = 26u * 1024u;
        const uint32_t fixed = mpad + FZ_TABLE_BYTES + FZ_PEQ_BYTES(bits_nw);
        // Queue entries per wave: one full pass (64) + twice the expected candidates per tile, within the LDS budget.
        uint32_t qc = sw().bits_qcap > 0 ? (uint32_t)sw().bits_qcap
                                         : (uint32_t)std::min(512.0, 64.0 + 32.0 * std::ceil(2.0 * per_tile / 32.0));
        while (qc > 64u && fixed + FZ_WAVES_PER_BLOCK * fz_wave_lds_pref_bytes(qc, fa.win_pieces) > budget) qc -= 32u;
        fa.qcap = qc;
        fused_lds = fixed + FZ_WAVES_PER_BLOCK * fz_wave_lds_pref_bytes(fa.qcap, fa.win_pieces);
        if (fused_lds > kFusedLdsBudget) bits_nw = 0;
        else fa.fused = 1u;
    }
    // Substitutions-only searches whose pattern lets expect dense candidates: the same Hamming count under the bit-vector forms' queue discipline — full 64-candidate passes, tiles denser than the queue
    // taken in block-range passes — instead of round 1's (half-full queues; a tile that overflows is enumerated: DNA, m = 20,
    // 4 substitutions: 14 ms per GiB; m = 12, 3: 45 ms).
    bool adapt_plain = false;
    if (!bits_nw && fa.fused && in_memory && with_verify && !sw().no_bits && per_tile > 16.0 && q.mode == FZ_MODE_SUBS) {
        const uint32_t fixed = mpad + FZ_TABLE_BYTES;
        uint32_t qc = sw().bits_qcap > 0 ? (uint32_t)sw().bits_qcap : (uint32_t)std::min(512.0, 64.0 + 32.0 * std::ceil(2.0 * per_tile / 32.0));
        while (qc > 64u && fixed + FZ_WAVES_PER_BLOCK * fz_wave_lds_pref_bytes(qc, fa.win_pieces) > target + 4096) qc -= 32u;
        if (fixed + FZ_WAVES_PER_BLOCK * fz_wave_lds_pref_bytes(qc, fa.win_pieces) <= kFusedLdsBudget) {
            adapt_plain = true;
            fa.qcap = qc;
            fused_lds = fixed + FZ_WAVES_PER_BLOCK * fz_wave_lds_pref_bytes(qc, fa.win_pieces);
        }
    }
    const bool no_wf_fuse = sw().no_wf_fuse;                                    // test / measurement knob: the stand-alone kernel
    const uint32_t wf_fused_lds = mpad + FZ_TABLE_BYTES + FZ_WAVES_PER_BLOCK * fz_wave_lds_bytes(fz_wf_fused_dwords(fa.win_dwords, (uint32_t)vp.gw), 0, 1, true);
    // (in-memory searches only: the segmented instances of this form spill registers — the file API keeps the kernel of its own)
    // 32 lanes per candidate (budgets 8 .. 15): the fused form is 7-14 % behind scan + stand-alone kernel where candidates
    // are rare (1 GiB of text, m = 64, k = 8 / 12: 0.546 / 0.654 against 0.509 / 0.597 ms) and 1.25 .. 7.7 x ahead where they
    // are not (DNA, m = 100, k = 10, 4.5e4 candidates: 0.551 against 0.687 ms; m = 54, k = 8, 2.4e6: 2.70 against 20.7 ms —
    // the hit list outgrows its buffer and the search runs twice).  FZ_WF32=0 / 1 pins the choice.
    const int wf32_env = sw().wf32;
    const bool wf_candidate = !bits_nw && !fa.fused && in_memory && with_verify && !force_big && !no_wf_fuse && vp.want_wf && !vp.big && vp.gw <= 32 &&
                              q.m <= FZ_MAX_M && wf_fused_lds <= target + 4096;
    // (round 6: patterns up to 128 characters never get here — bit-vector columns; for the longer ones the choice follows the
    //  expected density per_tile above, a function of the pattern — the measured crossover, 1.5e4 .. 4.5e4 candidates per GiB, is
    //  ~0.1 per tile and wave — not, as in rounds 4 and 5, what the context's previous search saw)
    const bool wf_fused = wf_candidate && (vp.gw == 16 || (wf32_env >= 0 ? wf32_env != 0 : per_tile > 0.1));
    if (wf_fused) { fa.fused = 1u; fused_lds = wf_fused_lds; fa.vlanes = 64; }
    sp.wfg = bits_nw ? bits_nw : adapt_plain ? 3 : wf_fused ? vp.gw : 0;
    sp.form = !with_verify ? FZ_FORM_NONE : bits_nw == 4 ? FZ_FORM_FUSED_BITS32 : bits_nw == 1 ? FZ_FORM_FUSED_BITS1 : bits_nw == 2 ? FZ_FORM_FUSED_BITS2
              : wf_fused ? FZ_FORM_FUSED_CELLS : fa.fused ? FZ_FORM_FUSED_BAND : FZ_FORM_KERNEL;
    // (the hit-emitting form keeps no pattern in LDS: fz_confirm reads it from the argument block / HBM)
    sp.lds = fa.fused ? fused_lds : FZ_TABLE_BYTES + FZ_WAVES_PER_BLOCK * fz_wave_lds_bytes(0, 0, 64, true);
    // Next to the predecessor: fused (no hit list), in memory, the pattern in the argument block (stage_pattern leaves the
    // HBM copy alone), whole-buffer scans (has_near_match_* never pipelines)
    sp.overlapped = shares_chip && fa.fused && in_memory && !partial && q.m <= FZ_MAX_M && !vp.big;

    // Grid: every workgroup strides over ~16 tiles (256 KiB).  Measured on MI355X at 1 GiB: 6 / 8 /
    // 12 / 16 / 20 / 32 / 64 workgroups per CU -> 0.302 / 0.302 / 0.276 / 0.267 / 0.265 / 0.280 /
    // 0.333 ms: several rounds of short workgroups overlap one workgroup's end-of-life verification
    // (latency-bound) with the others' streaming; too many pay the per-workgroup fixed cost.  At least
    // 6 per CU (the co-resident count at this kernel's SGPR use) so small inputs still fill the chip.
    // (Round 2 measured the alternative — a persistent grid whose waves draw 4 KiB chunks from ticket
    // counters so that all finish together: same time without candidates, 0.04 ms slower on DNA,
    // because every wave then runs its verification at the same moment, at the end.)
    // (re-measured with the software-pipelined loop of round 2, 1 GiB: 8 / 10 / 12 / 14 / 16 / 20 / 24 / 32 tiles ->
    //  DNA k = 2: 0.232 / 0.223 / 0.222 / 0.222 / 0.224 / 0.240 / 0.244 / 0.260 ms; exact search: 0.191 / 0.182 /
    //  0.187 / 0.193 / 0.199 / 0.201 / 0.196 / 0.205 ms)
    // Round 3 (two-level finish tickets in place, `profiles/r03_lab_ab.txt`): what matters below ~10 rounds of resident
    // workgroups is that the grid is a WHOLE number of rounds of 6 workgroups per CU (round 4's device stamps show SEVEN
    // resident per CU — amdgpu_waves_per_eu(7, 7) — so these are not rounds of residents; the multiples of 6 per CU
    // stay because they measured best, with and without the tapered last round below; a last round that is
    // 56 % full costs 1 GiB 8 us) of ~9.5 tiles per workgroup: 1 GiB, 4 rounds (10.7 tiles) 0.2046 ms, 5 rounds 0.2048,
    // 3 rounds 0.2062, 6 rounds 0.2074, 8 rounds 0.2104 against 0.2121-0.2146 for 12 tiles (3.56 rounds); 2 GiB, 9 rounds
    // 0.3887 against 0.3989; 512 MiB, 2 rounds 0.1165 against 0.1182.  Long inputs keep 12 tiles per workgroup (4 GiB:
    // 0.7743 against 0.7791-0.7855 for 14-18 whole rounds and 0.802 for 8 tiles: the per-workgroup cost wins there).
    constexpr uint64_t kTilesPerWg = 12;
    const uint64_t resident = (uint64_t)n_cus * 6;
    uint64_t max_grid = std::max<uint64_t>(resident, ntiles / kTilesPerWg);
    if (ntiles < resident * 120) {
        const uint64_t rounds = std::max<uint64_t>(1, (2 * ntiles + resident * 19 / 2) / (resident * 19));   // round(ntiles / (9.5 resident))
        max_grid = resident * rounds;
    }
    // A scan that runs next to its predecessor (sp.overlapped): 16 tiles per workgroup, no tapered last round.  The
    // older scan's drain is what the younger one fills, so neither the whole-rounds rule nor the taper has a drain of its
    // own to shorten; fewer, longer workgroups pay fewer per-workgroup costs.  Measured on MI355X, two searches in flight,
    // median ms per step (`profiles/r07_overlap.txt`), 1 GiB / 4 GiB: the plan of a scan alone 0.208-0.209 / 0.825-0.826;
    // taper off 0.205 / 0.819-0.820; 12 tiles 0.207 / 0.821-0.824; 16 tiles 0.205 / 0.808-0.809; 16 tiles, taper off
    // 0.201 / 0.804-0.805 (same box; on another 0.198 / 0.793, against 20 tiles 0.199 / 0.798, 24 tiles 0.203 / 0.811,
    // 32 tiles 0.200 / 0.801).
    constexpr uint64_t kTilesPerWgOverlapped = 16;
    constexpr bool kTaperOverlapped = false;
    if (sp.overlapped) max_grid = std::max<uint64_t>(resident, ntiles / kTilesPerWgOverlapped);
    // (has_near_match_*, measured in round 5 on 4 GiB with a match in the first MiB: 0.21 ms against 0.84 ms for the full
    //  scan.  What is left is NOT the running workgroups finishing their tiles but the ~21 800 workgroups that start after
    //  the first record, skip their tiles and still take their finish tickets: ~100 agent-scope atomics per microsecond on
    //  the sixteen shard words, which share one cache line.  Tried and dropped: a check of the record counter per tile in
    //  the scan's loop (cannot shorten what the tickets bound); workgroups of 6 tiles (0.31 ms: twice the tickets); the shard
    //  words spread over four lines of the header (every scan slower — 1 GiB exact search 0.188-0.193 -> 0.197 ms, same
    //  box: those lines also hold the statistics words).)
    // the queue codes carry a bounded per-workgroup tile iteration
    const uint64_t min_grid = (ntiles + FZ_TITER_MAX - 1) / FZ_TITER_MAX;
    sp.grid = (uint32_t)std::max<uint64_t>(std::max<uint64_t>(1, min_grid), std::min<uint64_t>(ntiles, max_grid));
    // Tapered last round: workgroups start in blockIdx order, so the last resident round of a launch starts while the
    // machine is still full and — with equal shares — ends one workgroup life (~60 us) after the grid ran dry, the chip
    // draining all the while (device stamps of every workgroup, benchmarks/lab_scan_phases.py: residency falls linearly from
    // 1 792 to 0 over the last 60 us of a 1 GiB launch).  The last `resident` workgroups therefore take shrinking shares
    // (kTaperSteps groups, down to kTaperMin of a full share) of their own tile range at the end of the buffer, the others
    // correspondingly more.
    if (!sp.overlapped || kTaperOverlapped) plan_scan_regions(fa, ntiles, sp.grid, n_cus);
    else if (sw().scan_rounds) plan_scan_rounds(fa, ntiles, sp.grid, n_cus);
    else fa.nreg = 0;
    if (partial) {                                               // one region: the call's tiles, no taper
        fa.nreg = 1;
        fa.reg_wg0[0] = 0; fa.reg_nwg[0] = sp.grid; fa.reg_tile0[0] = tile_lo; fa.reg_end[0] = tile_hi;
    }
    return sp;
}

// The block fields of one scan launch that starts at block g0 of the search (fa.mask1 and fa.d2 set): the longest run of
// blocks (at most 8) whose distinct hashes land in distinct table slots under some multiplier.  One block always fits; equal
// n-grams (equal hashes) share a slot and raise FZ_FLAG_DUP_HASHES.  -> the number of blocks of the launch.
uint32_t fill_launch_blocks(FzScanArgs &fa, const Search &q, uint32_t g0, const HashGeom &hgeom) {
    const uint32_t L = q.plan.L, G = (uint32_t)q.plan.s.size();
    uint32_t hash_k = 0, lut_shift = 0;
    const uint32_t nblk = choose_launch_blocks(q.p, q.plan.s.data(), g0, G, L, hash_k, lut_shift);
    fa.hash_k = hash_k;
    fa.lut_shift = lut_shift;
    fa.nblk = nblk;
    fa.g0 = g0;
    for (uint32_t b = 0; b < nblk; ++b) {
        const uint8_t *ng = q.p + q.plan.s[g0 + b];
        fa.A[b] = load_le32(ng, L) & fa.mask1;
        fa.B[b] = hgeom.nwin == 2 ? load_le32(ng + fa.d2, 4) : 0;
        fa.H[b] = hgeom.nwin == 2 ? fz_hash_windows(fa.A[b], load_le32(ng + hgeom.dh, 3), fa.hash_k) : fz_hash_short(fa.A[b], fa.hash_k);
        fa.s[b] = q.plan.s[g0 + b];
        fz_block_range(q.mode, q.m, q.k, L, fa.s[b], fa.lo_rel[b], fa.hi_sub[b]);
    }
    fa.flags = q.any ? FZ_FLAG_ANY : 0u;
    for (uint32_t b = 1; b < nblk; ++b)
        for (uint32_t c = 0; c < b; ++c)
            if (fa.H[b] == fa.H[c]) fa.flags |= FZ_FLAG_DUP_HASHES;
    return nblk;
}

// Enqueue scan (+ separate verify when it cannot be fused) for one shard on its device stream, as plan_scan decided.
// No host synchronisation.  `behind`: another search of the context is in flight (fz_*_begin with one search pending).
// `forward`: the re-run of a search whose results outgrew their buffers — always forward, so that the direction of a
// launch depends on nothing but the rule below.
int enqueue_shard(fz_ctx *ctx, const Shard &sh, const Search &q, bool with_verify, bool copy_back = true, bool behind = false,
                  bool forward = false) {
    DevState &d = lane_dev(ctx, sh.dev);
    HIP_TRY(hipSetDevice(d.device));
    unsigned long long *counters = reinterpret_cast<unsigned long long *>(d.d_out);
    FzRec *recs = reinterpret_cast<FzRec *>(d.d_out + kHeaderBytes);
    const bool no_direct = env_no_direct();
    // direct mode needs a kernel to publish the counters: an empty buffer launches none
    const bool snapshot = copy_back && with_verify && q.collective;      // collective search: records stay on the device
    const bool direct = copy_back && d.direct && !no_direct && !snapshot && sh.geom.buf_len > 0 && !q.plan.s.empty();
    if (direct && with_verify) recs = reinterpret_cast<FzRec *>(d.cur().h_stage_dev + kHeaderBytes);
    SearchRun &run = d.cur().run = SearchRun{};
    run.last_direct = direct;
    run.timed = ctx->timing;

    FzScanArgs fa;
    fill_common_args(fa, sh, q);
    const ScanPlan sp = plan_scan(q, sh.geom, (uint32_t)d.n_cus, with_verify, behind && ctx->streams == 2 && direct, fa);
    const VerifyPlan &vp = sp.vp;
    const uint32_t L = q.plan.L;
    const uint32_t G = (uint32_t)q.plan.s.size();
    const uint64_t ntiles = sp.ntiles;
    // (the scan kernel keeps a workgroup's distance to its limit and its signed tile stride in 32 bits: 32 TiB per shard)
    if ((sh.geom.buf_len + FZ_TILE_BYTES - 1) / FZ_TILE_BYTES >> 31) return fail(FZ_EUNSUPPORTED, "a shard of 2^31 tiles or more");
    const dim3 grid(sp.grid);
    if (q.mode == FZ_MODE_GENERIC && !with_verify) fa.gen_dedup = d.gen_dedup_arg;      // the scan fills the window table (run_generic)
    {
        int rc = stage_pattern(d, fa, q.p, q.m, with_verify && vp.big);
        if (rc) return rc;
    }
    const HashGeom hgeom(L);
    const int nwin = hgeom.nwin, dh = hgeom.dh;
    fa.d2 = nwin == 2 ? std::min<uint32_t>(L, 8) - 4 : 0;
    fa.mask1 = hgeom.mask1;
    fa.mask2 = 0xffffffffu;
    fa.hit_cap = d.hit_cap;
    fa.rec_cap = direct ? kHostRecs : d.rec_cap;
    // The stream and the counter block of this search.  An overlapped scan (plan_scan: fused, direct, in memory, the pattern
    // in the argument block) takes the stream its predecessor — the search in the device's other result slot — does not
    // use; so do the counters: stream_alt has d_hdr_alt, d.stream the header of d_out.  Two scans may then run at once
    // because nothing one of them writes is read or written by the other:
    //  - d_hits: only the hit-list forms write it, never a fused scan; a predecessor that is not fused may use it, its
    //    overlapped successor does not.
    //  - d_out: an overlapped scan on d.stream uses its header as counters (zeroed in stream order by the memset below or
    //    by the publishing workgroup of the last search on d.stream) and writes no records there: direct mode puts them in
    //    the pinned slot.  The scan on stream_alt never touches d_out.
    //  - the pinned slots: every search writes the records and the published counters of its own result slot (the current
    //    one while enqueue runs; pending_begin swaps the slots around the launch).
    //  - d_hdr_alt: one search at a time on stream_alt (the two in flight are on different streams); its publishing
    //    workgroup zeroes it for the next one, which is ordered behind it on that stream.
    //  - pattern staging (d_pat): an overlapped scan reads the pattern from its argument block; a predecessor staged on
    //    d.stream keeps the buffer to itself.
    //  - fallback: a result set beyond the pinned slot (collect_shard) synchronises both streams before it grows d_out /
    //    d_hits and re-runs the search on d.stream in copy mode; while a device is out of direct mode a second search is not
    //    launched before the first is collected (pending_begin), so nothing overlaps until direct mode returns.
    // Synchronous calls, the first search of a pipeline and everything not overlapped stay on d.stream.
    if (sp.overlapped && fa.pat_g) return fail(FZ_EDEVICE, "internal: an overlapped scan with the pattern staged in HBM");
    const bool alt = sp.overlapped && !d.slots[d.slot_id ^ 1].run.on_alt;
    run.on_alt = alt;
    const hipStream_t st = alt ? d.stream_alt : d.stream;
    if (alt) counters = reinterpret_cast<unsigned long long *>(d.d_hdr_alt);
    else {
        if (!d.header_zeroed) HIP_TRY(hipMemsetAsync(d.d_out, 0, kHeaderBytes, d.stream));
        d.header_zeroed = false;
    }

    // When the scan's last launch is also the search's last kernel (fused verification, results written straight to
    // the host), the start / completion events ride on the kernels' own dispatch packets (launch)
    // instead of two extra packets around them: fewer packets on the critical path of a synchronous call, and
    // filter_ms becomes the kernels' own span.
    const bool ext_events = copy_back && direct && !(with_verify && !fa.fused) && ntiles > 0 && G > 0;
    // ... and whenever the scan launches a kernel at all, its start / end events (ev[0], ev[1]: fz_stats' filter_ms) ride
    // on the first / last launch as well instead of two packets of their own in front of and behind the scan
    const bool attach = ntiles > 0 && G > 0;
    if (ctx->timing && !attach) HIP_TRY(hipEventRecord(d.cur().ev[0], st));
    uint32_t launches = 0;
    // Direction (FZ_FLAG_REVERSE).  A resident sequence is scanned again and again, and a sweep that starts where the last
    // one ended re-reads the lines read last while they are still in the Infinity Cache; two sweeps in the same direction
    // re-use every line at the distance of the whole buffer.  Every eligible launch — in memory, one sequence, the whole
    // buffer: each verification form, both streams of the pipeline, the launches of a search of more than 16 blocks among
    // themselves — therefore takes the direction that starts at the end its shard's last whole scan stopped at.  Batches,
    // file chunks, the growing pieces of has_near_match_* and overflow re-runs go forward.  Results are ordered on the
    // host: the direction changes no row, and neither the plan nor the number of launches.
    const bool may_reverse = sh.geom.seg_stride == 0 && !geom_is_ragged(sh.geom) && !sp.partial && !q.any && !forward;
    for (uint32_t g0 = 0; g0 < G && ntiles > 0;) {
        // Blocks [g0, g0 + nblk) of this launch, the hash multiplier and whether two of the blocks hash alike
        const uint32_t nblk = fill_launch_blocks(fa, q, g0, hgeom);
        const bool reverse = may_reverse && (ctx->scan_dir == 2 || (ctx->scan_dir == 0 && sh.scan_at_end));
        if (reverse) { fa.flags |= FZ_FLAG_REVERSE; ctx->rev_launches.fetch_add(1, std::memory_order_relaxed); }
        if (!sp.partial) sh.scan_at_end = !reverse;
        // the final kernel of the search publishes the counters to the host (direct mode)
        const bool verify_follows = with_verify && !fa.fused;
        fa.host_hdr = (direct && !verify_follows && g0 + nblk >= G) ? reinterpret_cast<uint64_t>(d.cur().h_stage_dev) : 0;
        const bool ragged = geom_is_ragged(sh.geom);
        const bool seg = sh.geom.seg_stride != 0;
        ScanKernel kern = ragged ? batch_scan_kernel(nwin, dh, fa.fused != 0, fa.lut_shift == 2, sp.wfg)
                          : scan_is_lean(q.mode, q.k, fa, sp.wfg, seg, ragged) ? lean_scan_kernel(nwin, dh, fa.lut_shift == 2)
                          : scan_kernel(nwin, dh, fa.fused != 0, seg, fa.lut_shift == 2, sp.wfg);
        if (!kern) return fail(FZ_EUNSUPPORTED, "this (lab) build carries no scan kernel for nwin=%d dh=%d", nwin, dh);
        hipEvent_t ev_start = (attach && ctx->timing && g0 == 0) ? d.cur().ev[0] : nullptr;
        hipEvent_t ev_stop = g0 + nblk >= G ? (ext_events ? d.cur().ev[3] : (attach && ctx->timing) ? d.cur().ev[1] : nullptr) : nullptr;
        launch(kern, grid, dim3(FZ_FILTER_THREADS), sp.lds, st, ev_start, ev_stop, sh.d_buf, fa, ntiles, d.d_hits, recs, counters);
        HIP_TRY(hipGetLastError());
        ++launches;
        g0 += nblk;
    }
    // ev[1] = end of the scan.  When the results need no copy and no verify kernel follows, ev[3] is
    // recorded at the same point of the stream: one event packet less on the critical path.
    run.scan_end_event = (copy_back && direct && !(with_verify && !fa.fused)) ? 3 : 1;
    if (run.scan_end_event == 1 && ctx->timing && !attach) HIP_TRY(hipEventRecord(d.cur().ev[1], st));
    // the verification kernel is the search's last one when its records go straight to the host: then the completion
    // event rides on its launch (no ev[2] / ev[3] packets behind it; the verify span is ev[1] .. ev[3])
    hipEvent_t v_stop = (copy_back && direct && !snapshot) ? d.cur().ev[3] : nullptr;
    if (with_verify && !fa.fused && ntiles > 0 && G > 0) {
        run.verify_launched = true;
        if (v_stop) run.verify_end_event = 3;
        fa.nblk = 0;
        fa.g0 = 0;
        fa.host_hdr = direct ? reinterpret_cast<uint64_t>(d.cur().h_stage_dev) : 0;
        using VerifyKernel = void (*)(const uint8_t *, const FzScanArgs, const uint64_t *, FzRec *, unsigned long long *);
        VerifyKernel vk;
        dim3 vgrid, vblock;
        size_t vlds;
        if (vp.big) {
            if (!fa.pat_g) return fail(FZ_EDEVICE, "internal: the pattern was not staged for the big verification");
            const uint32_t cells = q.mode == FZ_MODE_LEV ? 2 * q.k + 1 : 1;
            const bool rag = geom_is_ragged(sh.geom);
            if (cells <= 64) vk = rag ? fz_batch_verify_big_kernel<1> : fz_verify_big_kernel<1>;
            else if (cells <= 128) vk = rag ? fz_batch_verify_big_kernel<2> : fz_verify_big_kernel<2>;
            else if (cells <= 256) vk = rag ? fz_batch_verify_big_kernel<4> : fz_verify_big_kernel<4>;
            // (a batch takes the 16-cells-per-lane instance here as well — a wider band is as exact: the ragged instance
            //  with 8 cells per lane is the one kernel hipcc gives a 36-byte private segment, and no kernel of this library
            //  uses scratch memory)
            else if (cells <= 512) vk = rag ? fz_batch_verify_big_kernel<16> : fz_verify_big_kernel<8>;
            else if (cells <= 1024) vk = rag ? fz_batch_verify_big_kernel<16> : fz_verify_big_kernel<16>;
            else vk = rag ? fz_batch_verify_big_kernel<32> : fz_verify_big_kernel<32>;
            vgrid = dim3(d.n_cus * 32); vblock = dim3(64); vlds = 0;
        } else if (vp.want_wf) {
            // lane-per-cell: 64 / gw candidates per wave, one contiguous byte window per candidate
            fa.gw = (uint32_t)vp.gw;
            const bool rag = geom_is_ragged(sh.geom);
            if (vp.gw == 16) vk = rag ? fz_batch_verify_wf_kernel<16> : fz_verify_wf_kernel<16>;
            else if (vp.gw == 32) vk = rag ? fz_batch_verify_wf_kernel<32> : fz_verify_wf_kernel<32>;
            else vk = rag ? fz_batch_verify_wf_kernel<64> : fz_verify_wf_kernel<64>;
            // 16 waves per workgroup: few workgroups = few finish tickets (every ticket is an atomic on one word)
            vgrid = dim3(d.n_cus * 2); vblock = dim3(1024); vlds = vp.wf_lds;
        } else {
            // LDS: pattern + per-wave window and score ring; the block was shrunk until it fits.
            fa.vlanes = 64;
            vk = geom_is_ragged(sh.geom) ? fz_batch_verify_kernel : fz_verify_kernel;
            if (vp.ring_lds > 64 * 1024)
                HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(vk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)vp.ring_lds));
            vgrid = dim3(d.n_cus * 4); vblock = dim3(64 * vp.waves); vlds = vp.ring_lds;
        }
        launch(vk, vgrid, vblock, (uint32_t)vlds, d.stream, nullptr, v_stop, sh.d_buf, fa, d.d_hits, recs, counters);
        HIP_TRY(hipGetLastError());
    }
    const bool completion_attached = ext_events || (run.verify_launched && v_stop);
    if (copy_back) {
        if (run.verify_launched && ctx->timing && run.verify_end_event == 2) HIP_TRY(hipEventRecord(d.cur().ev[2], d.stream));
        if (snapshot) {
            // counters to the host (overflow checks, statistics); counters + records to this slot's snapshot
            HIP_TRY(hipMemcpyAsync(d.cur().h_stage, d.d_out, kHeaderBytes, hipMemcpyDeviceToHost, d.stream));
            int rc = ensure_send(d, d.rec_cap);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(d.cur().d_send, d.d_out, kHeaderBytes + d.rec_cap * sizeof(FzRec), hipMemcpyDeviceToDevice, d.stream));
            HIP_TRY(hipEventRecord(d.cur().ev_snap, d.stream));
            d.cur().snap_taken = true;
        } else if (!direct) {
            d.first_copy = std::min<uint64_t>(std::min<uint64_t>(d.first_copy, kFirstCopyRecs), d.rec_cap);
            HIP_TRY(hipMemcpyAsync(d.cur().h_stage, d.d_out, kHeaderBytes + d.first_copy * sizeof(FzRec), hipMemcpyDeviceToHost,
                                   d.stream));
        }
        if (!completion_attached) HIP_TRY(hipEventRecord(d.cur().ev[3], st));
        // the counters are zeroed for the NEXT search now, off the critical path of that call: by the
        // publishing workgroup itself in direct mode, by a memset behind the copy otherwise
        if (!direct) HIP_TRY(hipMemsetAsync(d.d_out, 0, kHeaderBytes, d.stream));
        if (!alt) d.header_zeroed = true;
    }
    run.launches_used = launches;                // (summed by search_enqueue: this may run on the device's worker thread)
    run.fused_used = fa.fused != 0;
    run.form_used = sp.form;
    run.hit_cap_used = d.hit_cap;
    run.rec_cap_used = d.rec_cap;
    return FZ_OK;
}

// Wait for a shard, handle overflow (so.rerun = capacities grown, the caller must re-run), collect into `so`.
// May run on the device's worker thread: touches the device state, `so` and — only for single-shard searches
// (view_ok), which never run on a worker — the context's record view.
int collect_shard(fz_ctx *ctx, const Shard &sh, bool with_verify, bool view_ok, ShardOut &so, bool collective = false) {
    DevState &d = ctx->devs[sh.dev];
    const SearchRun &run = d.cur().run;
    HIP_TRY(hipSetDevice(d.device));
    Trace tr;
    so.recs.clear();
    so.hits.clear();
    so.rerun = false;
    so.tref = {};
    so.nh = so.nr = so.bytes = 0;
    // wait for the copy only: the memset that pre-zeroes the header for the next search runs behind it
    HIP_TRY(hipEventSynchronize(d.cur().ev[3]));
    tr.mark("  sync");
    const unsigned long long *cnt = reinterpret_cast<const unsigned long long *>(d.cur().h_stage);
    uint64_t nh = cnt[0];
    const uint64_t nr = cnt[1];
    const bool fused = with_verify && run.fused_used;
    if (fused) { nh = 0; for (int i = 0; i < 64; ++i) nh += cnt[8 + i]; }
    bool rerun = false;
    if (nh > run.hit_cap_used && !fused) {
        HIP_TRY(hipStreamSynchronize(d.stream));          // a second search in flight still uses the old buffers
        HIP_TRY(hipStreamSynchronize(d.stream_alt));
        int rc = ensure_hits(d, nh + nh / 8 + 1024);
        if (rc) return rc;
        rerun = true;
    }
    if (run.last_direct && with_verify && nr > kHostRecs) d.direct = false;   // too many for the staging buffer
    if (nr > (run.last_direct ? kHostRecs : run.rec_cap_used)) {
        HIP_TRY(hipStreamSynchronize(d.stream));
        HIP_TRY(hipStreamSynchronize(d.stream_alt));
        int rc = ensure_recs(d, nr + nr / 8 + 1024);
        if (rc) return rc;
        rerun = true;
    }
    if (!run.last_direct && nr * 4 < kHostRecs) d.direct = true;
    so.rerun = rerun;
    if (rerun) return FZ_OK;
    d.last_filter_ms = 0;
    if (run.timed) so.tref = timing_ref(d, /*generic=*/false);
    so.bytes = sh.geom.buf_len;
    so.nh = nh;
    if (with_verify && collective) {
        // collective search: the records travel in the all-gather (gather_records), not through this host
    } else if (with_verify && view_ok && run.last_direct) {
        so.nr = nr;
        ctx->view = reinterpret_cast<const FzRec *>(d.cur().h_stage + kHeaderBytes);
        ctx->view_n = nr;
    } else if (with_verify) {
        so.nr = nr;
        so.recs.resize(nr);
        const uint64_t first = run.last_direct ? nr : std::min<uint64_t>(nr, d.first_copy);
        if (first) memcpy(so.recs.data(), d.cur().h_stage + kHeaderBytes, first * sizeof(FzRec));
        if (nr > first)
            HIP_TRY(hipMemcpy(so.recs.data() + first, d.d_out + kHeaderBytes + first * sizeof(FzRec),
                              (nr - first) * sizeof(FzRec), hipMemcpyDeviceToHost));
        d.first_copy = std::max<uint64_t>(512, nr + nr / 4 + 64);      // next call: fetch about this many
    } else {
        so.hits.resize(nh);
        if (nh) HIP_TRY(hipMemcpy(so.hits.data(), d.d_hits, nh * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    return FZ_OK;
}

int check_halo(const fz_seq *seq, uint64_t need) {
    for (const Shard &sh : seq->shards) {
        const FzGeom &g = sh.geom;
        const uint64_t want_lo = g.own_lo > need ? g.own_lo - need : 0;
        const uint64_t want_hi = std::min<uint64_t>(g.n, g.own_hi + need);
        if (g.own_hi > g.own_lo && (g.buf_off > want_lo || g.buf_off + g.buf_len < want_hi))
            return fail(FZ_EHALO, "shard halo too small: need %llu bytes around [%llu, %llu)",
                        (unsigned long long)need, (unsigned long long)g.own_lo, (unsigned long long)g.own_hi);
    }
    return FZ_OK;
}

// fn(si) for every shard of the sequence: on the shard's device worker when the context has workers and the sequence
// several shards (one shard per device), else on the calling thread in shard order.  -> first error.
template <class F>
int for_each_shard(fz_ctx *ctx, fz_seq *seq, F fn) {
    const size_t ns = seq->shards.size();
    if (!ctx->workers || ns < 2) {
        for (size_t si = 0; si < ns; ++si) { int rc = fn(si); if (rc) return rc; }
        return FZ_OK;
    }
    for (size_t si = 0; si < ns; ++si) ctx->workers->post((size_t)seq->shards[si].dev, [fn, si]() { return fn(si); });
    int rc = FZ_OK;
    std::string err;
    for (size_t si = 0; si < ns; ++si) {
        const int r = ctx->workers->wait((size_t)seq->shards[si].dev);
        if (r && !rc) { rc = r; err = g_err; }
    }
    if (rc) g_err = err;
    return rc;
}

int comm_rank_lows(fz_ctx *ctx, fz_seq *seq);
int comm_gather_host(fz_ctx *ctx, const void *data, uint64_t bytes, std::vector<uint8_t> &all);
int comm_or(fz_ctx *ctx, bool &flag);
bool comm_multi_process(const fz_ctx *ctx);

// Host half of the exchange step: `blocks` = world blocks of `bytes_per_rank` bytes, each [1 KiB of counters][records];
// counters[1] = records the rank produced (it stored min(count, cap) of them).  -> *top = the largest count; if it is
// above `cap` nothing else happens (the caller re-gathers with a larger capacity: every rank sees the same headers and
// decides alike).  Else `recs` = the ranks' records rank by rank, seg_ends[r] = where rank r's end, seg_order = the
// ranks in ascending order of the index range they own (own_lo[r]; a rank that owns nothing sorts by its number).
void parse_gathered(const uint8_t *blocks, int world, uint64_t bytes_per_rank, uint64_t cap, const uint64_t *own_lo,
                    std::vector<FzRec> &recs, std::vector<size_t> &seg_ends, std::vector<uint32_t> &seg_order, uint64_t *top_out,
                    uint64_t *total_out) {
    uint64_t top = 0, total = 0;
    for (int r = 0; r < world; ++r) {
        const unsigned long long *cnt = reinterpret_cast<const unsigned long long *>(blocks + (uint64_t)r * bytes_per_rank);
        top = std::max<uint64_t>(top, cnt[1]);
        total += cnt[1];
    }
    *top_out = top;
    *total_out = total;
    recs.clear();
    seg_ends.clear();
    seg_order.clear();
    if (top > cap) return;
    recs.resize(total);
    uint64_t o = 0;
    for (int r = 0; r < world; ++r) {
        const uint8_t *blk = blocks + (uint64_t)r * bytes_per_rank;
        const uint64_t c = reinterpret_cast<const unsigned long long *>(blk)[1];
        if (c) memcpy(recs.data() + o, blk + kHeaderBytes, c * sizeof(FzRec));
        o += c;
        seg_ends.push_back(o);
        seg_order.push_back((uint32_t)r);
    }
    if (own_lo)
        std::stable_sort(seg_order.begin(), seg_order.end(), [&](uint32_t x, uint32_t y) { return own_lo[x] < own_lo[y]; });
}

// RCCL is loaded on first use (dlopen), not linked: a single-GPU install without librccl — or with ROCM_PATH pointing
// somewhere that lacks it — still loads libfzhip.so and searches; only fz_comm_* then return FZ_EUNSUPPORTED.
struct RcclApi {
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string error;
    bool ok = false;
    bool stand_in = false;                       // tests/mock_rccl.cpp (FZ_RCCL_LIB): N ranks on ONE device are possible
};

const RcclApi *rccl_api() {
    static const RcclApi api = []() {
        RcclApi a;
        if (sw().no_rccl) { a.error = "disabled by FZ_NO_RCCL"; return a; }      // test knob: an install without librccl
        std::vector<std::string> names;
        if (!sw().rccl_lib.empty()) names.push_back(sw().rccl_lib);
        names.push_back("librccl.so.1");
        names.push_back("librccl.so");
        names.push_back(sw().rocm_path + "/lib/librccl.so.1");
        void *h = nullptr;
        for (const std::string &n : names) {
            h = dlopen(n.c_str(), RTLD_NOW | RTLD_GLOBAL);
            if (h) break;
            const char *de = dlerror();
            a.error += (a.error.empty() ? "" : "; ") + std::string(de ? de : n.c_str());
        }
        if (!h) return a;
        bool all = true;
        auto sym = [&](const char *name) { void *p = dlsym(h, name); if (!p) { all = false; a.error = std::string("librccl lacks ") + name; } return p; };
        a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(sym("ncclGetUniqueId"));
        a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(sym("ncclCommInitRank"));
        a.CommInitAll = reinterpret_cast<decltype(a.CommInitAll)>(sym("ncclCommInitAll"));
        a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(sym("ncclCommDestroy"));
        a.AllGather = reinterpret_cast<decltype(a.AllGather)>(sym("ncclAllGather"));
        a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(sym("ncclAllReduce"));
        a.GroupStart = reinterpret_cast<decltype(a.GroupStart)>(sym("ncclGroupStart"));
        a.GroupEnd = reinterpret_cast<decltype(a.GroupEnd)>(sym("ncclGroupEnd"));
        a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(sym("ncclGetErrorString"));
        a.ok = all;
        a.stand_in = dlsym(h, "fzmock_rccl") != nullptr;
        return a;
    }();
    return &api;
}

#define RCCL_NEED()                                                                                \
    do {                                                                                           \
        if (!rccl_api()->ok) return fail(FZ_EUNSUPPORTED, "RCCL is not available (%s)", rccl_api()->error.c_str()); \
    } while (0)

#define NCCL_TRY(expr)                                                                             \
    do {                                                                                           \
        ncclResult_t r_ = (expr);                                                                  \
        if (r_ != ncclSuccess) return fail(FZ_EDEVICE, "%s failed: %s", #expr, rccl_api()->GetErrorString(r_)); \
    } while (0)

// Every wait for a collective has a deadline (FZ_COMM_TIMEOUT_MS, default 60 s): a rank that never arrives — a peer process
// that died, a link that does not come up — is an error the caller can act on (bench.py prints its line with
// `collective_error` and the host-merged value), not a job that hangs until somebody kills it.  Polling (hipStreamQuery)
// instead of hipStreamSynchronize: spinning at first — a gather takes tens of microseconds —, yielding after 200 us.
int comm_wait(hipStream_t st, const char *what) {
    const auto t0 = std::chrono::steady_clock::now();
    const long limit_ms = sw().comm_timeout_ms;
    for (;;) {
        const hipError_t e = hipStreamQuery(st);
        if (e == hipSuccess) return FZ_OK;
        (void)hipGetLastError();                           // (hipErrorNotReady is an answer, not a failure of a later launch)
        if (e != hipErrorNotReady) return fail(FZ_EDEVICE, "%s: %s", what, hipGetErrorString(e));
        const auto waited = std::chrono::steady_clock::now() - t0;
        if (waited > std::chrono::milliseconds(limit_ms))
            return fail(FZ_ETIMEOUT, "%s did not complete within %ld ms (FZ_COMM_TIMEOUT_MS): a rank of the communicator never arrived",
                        what, limit_ms);
        if (waited > std::chrono::microseconds(200)) std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

// The exchange step of a sharded search: every rank of the communicator contributes the
// snapshot of its counters + records (FzRec, unordered), ONE ncclAllGather of kHeaderBytes + gcap records per
// rank (a group call over the device states of this process), one D2H copy of the gathered block, and every rank
// holds all records of the global search; the caller orders them by (block, index) as it does for one shard.
// gcap follows the counts: the gathered headers show every rank the same numbers, so all ranks grow / shrink
// alike; an overflow re-gathers from the same snapshots (they hold everything the search produced).
// The ranks' segments are ordered by the index ranges they own (exchanged once per sequence: comm_rank_lows).
int gather_records(fz_ctx *ctx, fz_seq *seq, std::vector<FzRec> &recs) {
    const int world = ctx->comm_world;
    if (world <= 0) return fail(FZ_EINVAL, "the context has not joined a communicator");
    if (ctx->comm_broken) return fail(FZ_ETIMEOUT, "the communicator was abandoned after a collective ran into its deadline: "
                                                   "fz_comm_set_collective(ctx, 0) searches without it");
    recs.clear();
    const auto t_start = std::chrono::steady_clock::now();
    int rcl = comm_rank_lows(ctx, seq);
    if (rcl) return rcl;
    for (int attempt = 0; attempt < 8; ++attempt) {
        const uint64_t bytes = kHeaderBytes + ctx->gcap * sizeof(FzRec);
        for (DevState &d : ctx->devs) {
            HIP_TRY(hipSetDevice(d.device));
            int rc = ensure_send(d, std::max<uint64_t>(d.rec_cap, ctx->gcap));
            if (rc) return rc;
            if (d.recv_bytes < (uint64_t)world * bytes) {
                HIP_TRY(hipStreamSynchronize(d.comm_stream));
                if (d.d_recv) HIP_TRY(hipFree(d.d_recv));
                if (d.h_recv) HIP_TRY(hipHostFree(d.h_recv));
                d.d_recv = nullptr; d.h_recv = nullptr; d.recv_bytes = 0;
                HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d.d_recv), (uint64_t)world * bytes));
                HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&d.h_recv), (uint64_t)world * bytes, hipHostMallocDefault));
                d.recv_bytes = (uint64_t)world * bytes;
            }
            bool has_shard = false;
            for (const Shard &sh : seq->shards) has_shard |= &ctx->devs[sh.dev] == &d;
            if (has_shard && d.cur().snap_taken) HIP_TRY(hipStreamWaitEvent(d.comm_stream, d.cur().ev_snap, 0));
            else HIP_TRY(hipMemsetAsync(d.cur().d_send, 0, kHeaderBytes, d.comm_stream));   // this rank holds nothing of the sequence
        }
        NCCL_TRY(rccl_api()->GroupStart());
        for (DevState &d : ctx->devs)
            NCCL_TRY(rccl_api()->AllGather(d.cur().d_send, d.d_recv, bytes, ncclChar, d.comm, d.comm_stream));
        NCCL_TRY(rccl_api()->GroupEnd());
        DevState &d0 = ctx->devs[0];
        HIP_TRY(hipSetDevice(d0.device));
        HIP_TRY(hipMemcpyAsync(d0.h_recv, d0.d_recv, (uint64_t)world * bytes, hipMemcpyDeviceToHost, d0.comm_stream));
        HIP_TRY(hipEventRecord(d0.ev_done, d0.comm_stream));
        {
            int rcw = comm_wait(d0.comm_stream, "the all-gather of the ranks' records");
            if (rcw) { if (rcw == FZ_ETIMEOUT) ctx->comm_broken = true; return rcw; }
        }
        for (size_t i = 1; i < ctx->devs.size(); ++i) {      // the other device states of this process: only wait
            HIP_TRY(hipSetDevice(ctx->devs[i].device));
            int rcw = comm_wait(ctx->devs[i].comm_stream, "the all-gather of the ranks' records");
            if (rcw) { if (rcw == FZ_ETIMEOUT) ctx->comm_broken = true; return rcw; }
        }
        uint64_t top = 0, total = 0;
        parse_gathered(d0.h_recv, world, bytes, ctx->gcap, seq->rank_lo.data(), recs, ctx->seg_ends, ctx->seg_order, &top, &total);
        if (top > ctx->gcap) {                               // identical decision on every rank
            ctx->gcap = (top + top / 4 + 1023) / 1024 * 1024;
            continue;
        }
        ctx->stats.raw_matches = total;
        const uint64_t want = std::max<uint64_t>(1024, (top + top / 4 + 1023) / 1024 * 1024);
        if (want * 2 <= ctx->gcap) ctx->gcap = want;         // follow the counts down as well (hysteresis: a factor of two)
        ctx->last_gather_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
        return FZ_OK;
    }
    return fail(FZ_EDEVICE, "all-gather capacity kept overflowing");
}

// Launch a search on every shard (no host synchronisation).
int search_enqueue(fz_ctx *ctx, fz_seq *seq, const Search &q, bool with_verify, bool behind = false, bool forward = false) {
    ctx->view = nullptr;
    ctx->view_n = 0;
    ctx->rows_ready = false;
    ctx->stats.filter_launches = 0;
    ctx->stats.bytes_scanned = ctx->stats.ngram_hits = ctx->stats.raw_matches = 0;
    ctx->stats.filter_ms = ctx->stats.verify_ms = ctx->stats.device_ms = 0;
    ctx->tref.clear();
    int rc = for_each_shard(ctx, seq, [ctx, seq, &q, with_verify, behind, forward](size_t si) {
        return enqueue_shard(ctx, seq->shards[si], q, with_verify, true, behind, forward);
    });
    if (rc) return rc;
    for (const Shard &sh : seq->shards) {
        const SearchRun &run = lane_dev(ctx, sh.dev).cur().run;
        ctx->stats.filter_launches += run.launches_used;
        ctx->stats.verify_form = run.form_used;
    }
    return FZ_OK;
}

int emit_matches(const FzRec *recs, size_t cnt, uint32_t L, fz_match **out, uint64_t *n, uint64_t idx_bound, uint32_t blk_bound,
                 bool may_have_empty, std::vector<fz_match> *into);

// Wait for the search launched by search_enqueue and collect it; on an overflow the buffers have
// been grown and the search is launched again (deterministic, at most three times).
// One shard: the records are in `recs` (or the context's view of the staging buffer), the hits in `hits`.
// Several shards: every shard's records are collected AND ordered on its own (ctx->souts[si].rows, by the device's
// worker when the context has workers) and emit_matches only merges the rows (ctx->rows_ready); hits are concatenated.
int search_collect(fz_ctx *ctx, fz_seq *seq, const Search &q, bool with_verify, std::vector<FzRec> &recs,
                   std::vector<uint64_t> &hits) {
    const size_t ns = seq->shards.size();
    if (ctx->souts.size() < ns) ctx->souts.resize(ns);
    const bool order_rows = with_verify && !q.collective && ns > 1 && !q.any && seq->shards[0].geom.seg_stride == 0;
    for (int attempt = 0; attempt < 4; ++attempt) {
        recs.clear();
        hits.clear();
        ctx->rows_ready = false;
        // the statistics describe the search being collected (a younger one may have been launched meanwhile)
        ctx->stats.bytes_scanned = ctx->stats.ngram_hits = ctx->stats.raw_matches = 0;
        ctx->stats.filter_ms = ctx->stats.verify_ms = ctx->stats.device_ms = 0;
        ctx->tref.clear();
        Trace tr;
        ctx->seg_ends.clear();
        ctx->seg_order.clear();
        const uint32_t L = q.plan.L, nblk = (uint32_t)q.plan.s.size();
        const uint64_t nglob = seq->n;
        const bool collective = q.collective;
        int rc = for_each_shard(ctx, seq, [ctx, seq, with_verify, ns, collective, order_rows, L, nblk, nglob](size_t si) {
            ShardOut &so = ctx->souts[si];
            int r = collect_shard(ctx, seq->shards[si], with_verify, ns == 1, so, collective);
            if (r || so.rerun || !order_rows) return r;
            const bool dense = ctx->devs[seq->shards[si].dev].cur().run.fused_used;
            return emit_matches(so.recs.data(), so.recs.size(), L, nullptr, nullptr, nglob, nblk, !dense, &so.rows);
        });
        if (rc) return rc;
        bool any_rerun = false;
        for (size_t si = 0; si < ns; ++si) {
            ShardOut &so = ctx->souts[si];
            any_rerun |= so.rerun;
            if (so.rerun) continue;
            ctx->stats.bytes_scanned += so.bytes;
            ctx->stats.ngram_hits += so.nh;
            ctx->stats.raw_matches += so.nr;
            if (so.tref.d) ctx->tref.push_back(so.tref);
        }
        tr.mark(" collect");
        if (!any_rerun) {
            if (with_verify && q.collective) {
                int rc2 = gather_records(ctx, seq, recs);
                if (rc2) return rc2;
                tr.mark(" all-gather");
                return FZ_OK;
            }
            if (ns == 1) {
                recs.swap(ctx->souts[0].recs);
                hits.swap(ctx->souts[0].hits);
            } else if (order_rows) {
                ctx->rows_ready = true;
                for (uint32_t si = 0; si < ns; ++si) ctx->seg_order.push_back(si);
                std::sort(ctx->seg_order.begin(), ctx->seg_order.end(), [&](uint32_t x, uint32_t y) {
                    return seq->shards[x].geom.own_lo < seq->shards[y].geom.own_lo;
                });
            } else {
                for (size_t si = 0; si < ns; ++si) {
                    recs.insert(recs.end(), ctx->souts[si].recs.begin(), ctx->souts[si].recs.end());
                    hits.insert(hits.end(), ctx->souts[si].hits.begin(), ctx->souts[si].hits.end());
                }
            }
            return FZ_OK;
        }
        rc = search_enqueue(ctx, seq, q, with_verify, false, /*forward=*/true);
        if (rc) return rc;
    }
    return fail(FZ_EDEVICE, "result buffers kept overflowing");
}

int run_search(fz_ctx *ctx, fz_seq *seq, const Search &q, bool with_verify, std::vector<FzRec> &recs,
               std::vector<uint64_t> &hits) {
    if (ctx->npend) return fail(FZ_EINVAL, "a search started with fz_lev_ngrams_begin is still in flight");
    memset(&ctx->stats, 0, sizeof ctx->stats); ctx->tref.clear();
    ctx->stats.n_devices = (uint32_t)ctx->devs.size();
    Trace tr;
    int rc = search_enqueue(ctx, seq, q, with_verify);
    if (rc) return rc;
    tr.mark(" enqueue");
    return search_collect(ctx, seq, q, with_verify, recs, hits);
}

// fz_gen_hit_kernel's form for a generic search with `cand_cap` candidate slots per list.
using GhKernel = void (*)(const uint8_t *, const FzScanArgs, const uint64_t *, FzGenRec *, unsigned long long *);
struct GenHitPlan {
    GhKernel kernel;
    bool bits;                   // the bit-parallel form
    uint32_t waves;              // waves per hit
    uint32_t capw;               // slots per list of one wave
    size_t lds;
};

GenHitPlan plan_gen_hit(const Search &q, uint32_t cand_cap) {
    GenHitPlan g;
    const uint32_t mpad = (q.m + 15u) & ~15u, wpad = (q.m + 2 * q.k + 15u) & ~15u;
    // the bit-parallel form (fz_gen_hit_kernel<W, true>: 64-bit equality words, flags as words, unconditional stores):
    // patterns of at most 64 characters and budgets of at most 32.  FZ_GH_NO_BITS=1: the round-4 step (A/B, tests);
    // FZ_GH_WAVES=1 / 2 / 4: waves per hit.  Default with the bit-parallel form: ONE — measured in round 5 (profiles/
    // r05_generic_kernels.txt): a hit's time is ~1 500 cycles per window character that has candidates, whatever the
    // number of waves or of slices per trip (the big tree of a true occurrence belongs to one start, and the per-character
    // cost is the dependent chain of one trip), so more waves per hit only cost residency; 2 otherwise (round 4)
    // fz_gen_hit_kernel<W, true>'s implicit bounds, held HERE: one 64-bit equality word per window character (m <= 64),
    // the equality words of a window in two register pairs (m + 2k <= 128), skip counts in 32 bits (k <= 32), counters
    // below 2^31 (limits <= FZ_MAX_K = 255); anything else takes round 4's step
    static_assert(FZ_MAX_K < (1u << 31), "fz_b_lt / fz_b_eq operands");
    g.bits = q.m <= 64u && q.k <= 32u && q.m >= 1u && q.m + 2u * q.k <= 128u &&
             std::max(std::max(q.max_subs, q.max_ins), std::max(q.max_dels, q.k)) <= FZ_MAX_K && !sw().gh_no_bits;
    const uint32_t env = (uint32_t)sw().gh_waves;
    g.waves = env == 4u || env == 2u || (env == 1u && g.bits) ? env : g.bits ? 1u : 2u;
    g.capw = g.waves == 1u ? std::max<uint32_t>(64u, cand_cap) : std::max<uint32_t>(64u, cand_cap / 2u);
    g.lds = (size_t)mpad + wpad + FZ_GH_CTL_BYTES + (size_t)g.waves * 2u * g.capw * sizeof(FzGCand) +
            (size_t)g.waves * FZ_GH_MCAP_W(g.waves) * 8u +
            (g.bits ? (size_t)FZ_GH_PT_BYTES + (size_t)wpad * 8u + (size_t)64u * g.waves * 8u : 0u);
    g.kernel = g.bits ? (g.waves == 1u ? fz_gen_hit_kernel<1, true> : g.waves == 2u ? fz_gen_hit_kernel<2, true> : fz_gen_hit_kernel<4, true>)
                      : (g.waves == 4u ? fz_gen_hit_kernel<4, false> : fz_gen_hit_kernel<2, false>);
    return g;
}

// Generic search: scan (emit exact hits) -> fz_generic_kernel (one wave per hit) -> records.
// Re-runs with larger buffers on overflow: hit list, record list, then candidate lists.
// `phase`: 0 = the whole search; 1 = launch only (fz_generic_ngrams_begin: the kernels of the first attempt are enqueued on
// the current lane and the call returns); 2 = collect what phase 1 launched (fz_search_end), then carry on as phase 0 if
// a buffer turned out too small.
int run_generic(fz_ctx *ctx, fz_seq *seq, const Search &q, std::vector<FzGenRec> &recs_out, int phase = 0) {
    memset(&ctx->stats, 0, sizeof ctx->stats); ctx->tref.clear();
    ctx->stats.n_devices = (uint32_t)ctx->devs.size();
    static_assert(sizeof(FzGenRec) == sizeof(FzRec), "record buffers are shared");
    uint32_t cand_cap = ctx->gen_cand_cap;
    bool legacy_rest = false;                                  // the remaining attempts of this search use fz_lp_kernel
    for (int attempt = 0; attempt < 10; ++attempt) {
        recs_out.clear();
        ctx->any_found = false;
        ctx->gen_view = nullptr;
        ctx->gen_view_n = 0;
        ctx->gen_rows_dev = nullptr;
        ctx->gen_rows_n = 0;
        bool rerun = false;
        bool multi_failed = false, multi_ok = false;
        const bool legacy_now = legacy_rest || (attempt == 0 && phase != 2 && ctx->gen_multi_skip > 0);
        if (attempt == 0 && phase != 2 && ctx->gen_multi_skip > 0) { --ctx->gen_multi_skip; legacy_rest = true; }
        ctx->stats.filter_launches = 0;
        ctx->stats.bytes_scanned = ctx->stats.ngram_hits = ctx->stats.raw_matches = 0;
        ctx->stats.filter_ms = ctx->stats.verify_ms = ctx->stats.device_ms = 0;
        ctx->tref.clear();
        const uint32_t mpad = (q.m + 15u) & ~15u, wpad = (q.m + 2 * q.k + 15u) & ~15u;
        for (const Shard &sh : seq->shards) {
            if (phase == 2 && attempt == 0) break;            // launched by fz_generic_ngrams_begin
            DevState &d = lane_dev(ctx, sh.dev);
            // Window table: the hits that the n-gram blocks of one occurrence produce share their window, the automaton runs
            // once per window (fz_device.h: FzGenDedup; the scan fills the table as it lists the hits).  Where the rows are
            // finished on the device, where only (hull, best) pairs leave it, and for the flag-only search;
            // FZ_GEN_NO_DEDUP=1: every hit on its own (A/B, tests).
            // One shard, no segments: the rows are ordered and finished on the device (fz_gen_order_kernel,
            // fz_gen_scatter_kernel) and cross PCIe once, straight into the caller's buffer; the host's run ordering
            // (emit_generic) serves searches with more than FZ_GEN_ORDER_MAX hits, several shards and the file API's segments.
            const bool dev_order = !q.any && !q.fold && seq->shards.size() == 1 && sh.geom.seg_stride == 0 && !comm_multi_process(ctx);
            const bool dedup = !sw().gen_no_dedup && sh.geom.seg_stride == 0 && (dev_order || q.fold || q.any);
            d.gen_dedup_arg = 0;
            if (dedup) {
                HIP_TRY(hipSetDevice(d.device));
                if (!d.d_gen_dedup) {
                    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d.d_gen_dedup), FZ_GEN_DEDUP_BYTES));
                    d.dedup_zeroed = false;
                }
                if (!d.dedup_zeroed) HIP_TRY(hipMemsetAsync(d.d_gen_dedup, 0, FZ_GEN_DEDUP_ZERO_BYTES, d.stream));
                d.dedup_zeroed = false;
                d.gen_dedup_arg = reinterpret_cast<uint64_t>(d.d_gen_dedup);
            }
            int rc = enqueue_shard(ctx, sh, q, /*with_verify=*/false, /*copy_back=*/false, /*behind=*/false, /*forward=*/attempt > 0);   // (a re-run goes forward)
            if (rc) return rc;
            SearchRun &run = d.cur().run;                     // (fresh from enqueue_shard)
            run.dedup_used = dedup;
            size_t lds = 0;
            uint64_t scratch = 0;
            rc = cand_lists(d, cand_cap, mpad + wpad + FZ_GEN_MCAP * 8, lds, scratch);
            if (rc) return rc;
            FzScanArgs fa;
            fill_common_args(fa, sh, q);
            rc = stage_pattern(d, fa, q.p, q.m);
            if (rc) return rc;
            fa.flags = (q.any ? FZ_FLAG_ANY : 0u) | (q.fold ? FZ_FLAG_FOLD : 0u);
            fa.cand_cap = cand_cap;
            fa.cand_scratch = scratch;
            fa.lp_kind = FZ_LP_GENERIC_HIT;
            fa.lp_starts = 0;
            rc = ensure_big(d, 1u << 16);
            if (rc) return rc;
            fa.hit_cap = d.hit_cap;
            if (dev_order) {
                rc = ensure_gen_rows(d);
                if (rc) return rc;
                fa.gen_order = reinterpret_cast<uint64_t>(d.d_gen_order);
                fa.rows_cap = d.gen_rows_cap;
            }
            fa.gen_dedup = d.gen_dedup_arg;
            // Records of the automaton: into the device buffer, fetched with ONE copy once the count is known.
            // (Round 1 let the kernel store them straight into pinned host memory: 2.1e5 scattered 24-byte stores
            // cross PCIe at ~10 GB/s and the kernel cannot finish before they have drained — 0.49 ms for a kernel
            // whose work takes a fraction of that.)
            // Folded search (a few thousand pairs): the automaton kernel writes them straight into the pinned staging
            // buffer and its last workgroup publishes the counters there, as the fused scan does for its records — no
            // copy command between the kernel and the host (FZ_NO_DIRECT=1, or more pairs than the buffer holds: the copy).
            const bool fold_direct = q.fold && !env_no_direct() && d.fold_direct && seq->shards.size() == 1;
            run.fold_was_direct = fold_direct;
            fa.rec_cap = fold_direct ? kHostRecs : d.rec_cap;
            if (fold_direct) fa.host_hdr = reinterpret_cast<uint64_t>(d.cur().h_stage_dev);
            unsigned long long *counters = reinterpret_cast<unsigned long long *>(d.d_out);
            FzGenRec *recs = reinterpret_cast<FzGenRec *>((fold_direct ? d.cur().h_stage_dev : d.d_out) + kHeaderBytes);
            static_assert(sizeof(FzGenRec) == sizeof(FzRec), "the generic records share the record buffer");
            const GenHitPlan gp = plan_gen_hit(q, cand_cap);
            const bool multi = ctx->gen_multi && !legacy_now && scratch == 0 && sh.geom.seg_stride == 0 && gp.lds <= 160 * 1024;
            run.gen_multi_used = multi;
            if (multi) {
                fa.cand_cap = gp.capw;
                if (gp.lds > 64 * 1024)
                    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(gp.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)gp.lds));
            }
            const LpKernel lp = lp_kernel(FZ_LP_GENERIC_HIT, scratch != 0);
            if (lds > 64 * 1024)
                HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(lp), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            // (measured on configs[3b], 6144 hits: 16 / 24 / 32 workgroups per CU with 512-entry match buffers 0.325 /
            //  0.310 / 0.310 ms, with 128-entry ones 0.325 / 0.303 / 0.304 ms — once every hit is resident the kernel
            //  takes as long as its slowest hit)
            constexpr unsigned kLpGridPerCu = 24;
            // (configs[3b]: 16 -> 0.130 ms, 32 -> 0.104: every hit of the search needs a workgroup of its own)
            constexpr unsigned kGenHitGridPerCu = 32;
            // (Measured and NOT kept: for a search in flight next to another one, everything behind the scan on a HIGH-priority
            // stream of the lane, so that the automaton's waves take the slots the other lane's scan frees instead of waiting
            // behind its grid.  configs[3b], two in flight: 0.364 ms per search against 0.310 ms with the automaton on the
            // lane's own low-priority stream — the automaton's 4 171 waves then hold their CUs' registers for 160 us and the
            // scan, which is what bounds the pair, starves.)
            // the automaton's end event rides on its own launch; for a folded search in direct mode that event is also
            // the search's completion (ev[3]): no event packet of its own anywhere in such a search
            hipEvent_t lp_stop = fold_direct ? d.cur().ev[3] : ctx->timing ? d.cur().ev[2] : nullptr;
            run.lp_end_event = fold_direct ? 3 : 2;
            if (multi)
                launch(gp.kernel, dim3(d.n_cus * kGenHitGridPerCu), dim3(64 * gp.waves), (uint32_t)gp.lds, d.stream, nullptr, lp_stop,
                       sh.d_buf, fa, d.d_hits, recs, counters);
            else
                launch(lp, dim3(scratch ? kCandScratchGrid : d.n_cus * kLpGridPerCu), dim3(64), (uint32_t)lds, d.stream, nullptr, lp_stop,
                       sh.d_buf, fa, d.d_hits, (uint64_t)0, recs, counters);
            HIP_TRY(hipGetLastError());
            if (ctx->timing && !lp_stop && !fold_direct) HIP_TRY(hipEventRecord(d.cur().ev[2], d.stream));
            if (dev_order) {
                hipLaunchKernelGGL(fz_gen_order_kernel, dim3(d.n_cus * 8), dim3(256), 0, d.stream, d.d_hits, fa, counters);
                hipLaunchKernelGGL(fz_gen_scatter_kernel, dim3(d.n_cus * 8), dim3(256), 0, d.stream, d.d_hits, fa, recs,
                                   reinterpret_cast<FzOutRow *>(d.d_gen_rows), counters);
                HIP_TRY(hipGetLastError());
            }
            // folded search: the (few) pairs come back with the counters in ONE copy — as many as the previous search had
            run.fold_copied = fold_direct ? kHostRecs : q.fold ? std::min<uint64_t>(std::min<uint64_t>(d.fold_guess, kHostRecs), d.rec_cap) : 0;
            if (!fold_direct) {
                HIP_TRY(hipMemcpyAsync(d.cur().h_stage, d.d_out, kHeaderBytes + run.fold_copied * sizeof(FzGenRec), hipMemcpyDeviceToHost, d.stream));
                HIP_TRY(hipEventRecord(d.cur().ev[3], d.stream));
                // the counters are zeroed for the next search now, behind the copy (not in front of that search's scan)
                HIP_TRY(hipMemsetAsync(d.d_out, 0, kHeaderBytes, d.stream));
            } else {
                if (!lp_stop) HIP_TRY(hipEventRecord(d.cur().ev[3], d.stream));
            }
            d.header_zeroed = true;                           // (direct: by the publishing workgroup)
            if (dedup) {                                      // the window table is cleared for the next search, behind this one
                HIP_TRY(hipMemsetAsync(d.d_gen_dedup, 0, FZ_GEN_DEDUP_ZERO_BYTES, d.stream));
                d.dedup_zeroed = true;
            }
        }
        if (phase == 1) return FZ_OK;
        bool lists_overflowed = false;
        Trace trg;
        trg.mark(" generic enqueue");
        for (const Shard &sh : seq->shards) {
            DevState &d = lane_dev(ctx, sh.dev);
            const SearchRun &run = d.cur().run;
            HIP_TRY(hipSetDevice(d.device));
            HIP_TRY(hipEventSynchronize(d.cur().ev[3]));      // (recorded behind the last command of the search, on whichever stream)
            trg.mark(" generic sync");
            const unsigned long long *cnt = reinterpret_cast<const unsigned long long *>(d.cur().h_stage);
            const uint64_t nh = cnt[0], nr = cnt[1];
            uint64_t novf = cnt[2];
            if (run.gen_multi_used && cnt[FZ_HDR_GEN_FAIL]) { // a hit outgrew a wave's share of the list / its match buffer: one wave per hit
                multi_failed = true;
                if (q.any && nr > 0) { ctx->any_found = true; continue; }
                rerun = true;
                continue;
            }
            if (run.gen_multi_used) multi_ok = true;
            // rows of the ordered search: with the window table every hit takes its window's matches, computed once
            const uint64_t nrows = run.dedup_used && !q.fold && !q.any && nh <= FZ_GEN_ORDER_MAX ? cnt[FZ_HDR_GEN_ROWS] : nr;
            if (q.any) {                                      // has_near_match_generic_ngrams: a record anywhere settles it
                ctx->any_found |= nr > 0;
                if (nr > 0) continue;
                if (nh > d.hit_cap) { int rc = ensure_hits(d, nh + nh / 8 + 1024); if (rc) return rc; rerun = true; }
                if (novf) { lists_overflowed = true; rerun = true; }
                ctx->stats.bytes_scanned += sh.geom.buf_len;
                ctx->stats.ngram_hits += nh;
                continue;
            }
            if (nh > d.hit_cap) { int rc = ensure_hits(d, nh + nh / 8 + 1024); if (rc) return rc; rerun = true; }
            if (nr > d.big_cap) { int rc = ensure_big(d, nr + nr / 8 + 1024); if (rc) return rc; }
            if (run.fold_was_direct) {                        // pairs beyond the staging buffer were dropped: again, through d_out
                if (nr > kHostRecs) { d.fold_direct = false; rerun = true; }
            } else if (q.fold && nr * 4 < kHostRecs) d.fold_direct = true;
            if (!run.fold_was_direct && std::max(nr, nrows) > d.rec_cap) { int rc = ensure_recs(d, std::max(nr, nrows) + nrows / 8 + 1024); if (rc) return rc; rerun = true; }
            const bool rows_ready = !q.fold && seq->shards.size() == 1 && sh.geom.seg_stride == 0 &&
                                    nh <= FZ_GEN_ORDER_MAX && nrows <= d.gen_rows_cap && !comm_multi_process(ctx);
            // Window table + device ordering: only the windows' LEADERS left automaton records, the members' rows exist on the
            // device-ordered path alone.  If that path cannot be taken for this attempt (the row buffer is smaller than the row
            // count: the record buffers were regrown between the launch and this collection, e.g. by the other lane's search),
            // the host-ordered fallback below would silently miss the members' rows — run again, the launch sizes the row buffer
            // by the record capacity (ensure_gen_rows).  Not reachable with today's capacity bookkeeping (rows <= rec_cap is
            // checked above); kept as the invariant's enforcement.
            if (run.dedup_used && !q.fold && !q.any && !rows_ready && !rerun && nh <= FZ_GEN_ORDER_MAX && nrows > d.gen_rows_cap) {
                if (d.rec_cap < nrows) { int rc = ensure_recs(d, nrows + nrows / 8 + 1024); if (rc) return rc; }
                rerun = true;
            }
            const bool in_stage = q.fold && nr <= run.fold_copied && seq->shards.size() == 1;   // the pairs are in h_stage already
            if (q.fold) d.fold_guess = std::max<uint64_t>(4096, nr + nr / 4 + 256);
            if (!rerun && !novf && nr && !rows_ready && !in_stage)
                HIP_TRY(hipMemcpy(d.h_big, d.d_out + kHeaderBytes, nr * sizeof(FzGenRec), hipMemcpyDeviceToHost));
            if (novf) { lists_overflowed = true; rerun = true; }
            if (rerun) continue;
            if (run.timed) ctx->tref.push_back(timing_ref(d, /*generic=*/true));
            ctx->stats.bytes_scanned += sh.geom.buf_len;
            ctx->stats.ngram_hits += nh;
            if (rows_ready) {                                 // finished rows, fetched by emit_generic
                ctx->gen_rows_dev = d.d_gen_rows;
                ctx->gen_rows_n = nrows;
                ctx->gen_rows_device = d.device;
            } else if (seq->shards.size() == 1) {             // read in place (valid until the next search)
                ctx->gen_view = reinterpret_cast<const FzGenRec *>(in_stage ? d.cur().h_stage + kHeaderBytes : d.h_big);
                ctx->gen_view_n = nr;
            } else {
                const size_t base = recs_out.size();
                recs_out.resize(base + nr);
                if (nr) memcpy(recs_out.data() + base, d.h_big, nr * sizeof(FzGenRec));
            }
        }
        if (multi_failed) {
            legacy_rest = true;
            ctx->gen_multi_backoff = ctx->gen_multi_backoff ? std::min<uint32_t>(64u, ctx->gen_multi_backoff * 2u) : 1u;
            ctx->gen_multi_skip = ctx->gen_multi_backoff;
        } else if (multi_ok && !rerun) {
            ctx->gen_multi_backoff = 0;
        }
        if (lists_overflowed) cand_cap *= 4;
        if (q.any && ctx->any_found) return FZ_OK;
        if (!rerun) {
            ctx->gen_cand_cap = std::min<uint32_t>(cand_cap, kCandLdsMax);   // remember what worked, never the HBM fallback
            return FZ_OK;
        }
    }
    return fail(FZ_EUNSUPPORTED, "generic search: candidate lists / result buffers kept overflowing");
}

// Result buffers handed to the caller (released with fz_free).  Large ones (a generic search over 1 GiB of text
// returns 2.1e5 rows = 5 MB) are recycled: glibc serves them with mmap and gives them back with munmap, so every
// call would fault in ~1200 fresh pages while it writes the rows (~0.3 ms of a 1.4 ms call).  A header in front of
// the payload carries the capacity; fz_free parks up to two big blocks, alloc_out takes a parked block that fits.
struct OutHdr { uint64_t bytes; uint64_t magic; };
constexpr uint64_t kOutMagic = 0x667a6f7574627566ull;
constexpr uint64_t kOutRecycleMin = 32u << 10;
std::mutex g_out_lock;
OutHdr *g_out_parked[2] = {nullptr, nullptr};

int alloc_out(uint64_t n, size_t elem, void **out) {
    const uint64_t need = std::max<uint64_t>(1, n * elem);
    OutHdr *h = nullptr;
    if (need >= kOutRecycleMin) {
        std::lock_guard<std::mutex> g(g_out_lock);
        for (OutHdr *&slot : g_out_parked)
            if (slot && slot->bytes >= need && slot->bytes <= 4 * need) { h = slot; slot = nullptr; break; }
    }
    if (!h) {
        h = static_cast<OutHdr *>(malloc(sizeof(OutHdr) + need));
        if (!h) { *out = nullptr; return fail(FZ_ENOMEM, "out of host memory for %llu results", (unsigned long long)n); }
        h->bytes = need;
        h->magic = kOutMagic;
    }
    *out = h + 1;
    return FZ_OK;
}

void release_out(void *p) {
    if (!p) return;
    OutHdr *h = static_cast<OutHdr *>(p) - 1;
    if (h->magic != kOutMagic) { fprintf(stderr, "fz_free: not a libfzhip result buffer\n"); abort(); }
    if (h->bytes >= kOutRecycleMin) {
        std::lock_guard<std::mutex> g(g_out_lock);
        for (OutHdr *&slot : g_out_parked)
            if (!slot) { slot = h; return; }
    }
    h->magic = 0;
    free(h);
}

int validate(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, bool in_pipeline = false) {
    if (!ctx || !seq || seq->ctx != ctx) return fail(FZ_EINVAL, "bad ctx/seq handle");
    if (seq->is_batch != ctx->batch_call)
        return fail(FZ_EINVAL, seq->is_batch ? "a batch handle (fz_batch_upload) is searched with fz_batch_search only"
                                             : "fz_batch_search takes a batch handle (fz_batch_upload)");
    if (ctx->npend && !in_pipeline) return fail(FZ_EINVAL, "a search started with fz_lev_ngrams_begin is still in flight");
    if (ctx->stream_inflight) return fail(FZ_EINVAL, "a file stream of this context has a batch in flight (finish or close it first)");
    if (!p || m == 0) return fail(FZ_EINVAL, "subsequence must not be empty");
    if (m > FZ_MAX_M_ANY) return fail(FZ_EUNSUPPORTED, "subsequence longer than %u bytes", FZ_MAX_M_ANY);
    return FZ_OK;
}

// Order records by key = (block, idx): LSD radix sort over the key bytes that actually vary
// (O(M) — a comparison sort of the 24-byte records costs ~40 ns per record on the host).
void sort_recs(std::vector<FzRec> &recs) {
    const size_t n = recs.size();
    if (n < 2) return;
    if (n < 64) {
        std::sort(recs.begin(), recs.end(), [](const FzRec &a, const FzRec &b) { return a.key < b.key; });
        return;
    }
    uint64_t diff = 0;
    for (size_t i = 1; i < n; ++i) diff |= recs[i].key ^ recs[0].key;
    std::vector<FzRec> tmp(n);
    FzRec *src = recs.data(), *dst = tmp.data();
    for (int byte = 0; byte < 8; ++byte) {
        if (((diff >> (8 * byte)) & 0xff) == 0) continue;
        size_t count[257] = {0};
        for (size_t i = 0; i < n; ++i) ++count[((src[i].key >> (8 * byte)) & 0xff) + 1];
        for (int b = 0; b < 256; ++b) count[b + 1] += count[b];
        for (size_t i = 0; i < n; ++i) dst[count[(src[i].key >> (8 * byte)) & 0xff]++] = src[i];
        std::swap(src, dst);
    }
    if (src != recs.data()) memcpy(recs.data(), src, n * sizeof(FzRec));
}

// Records -> fz_match rows in (block, index) order == the reference's emission order.
// The keys of one search differ in few bits (block number + an index range), so they are first
// squeezed next to the record's position into one 64-bit word and those words are sorted with 11-bit
// LSD radix passes over the key bits only (8-byte elements instead of 24-byte records); the records
// are then read once, in order.
// Slot-per-hit kernels leave FZ_REC_NONE in the slots of hits that did not verify.
bool drop_empty_slots(const FzRec *recs, size_t cnt, std::vector<FzRec> &kept) {
    size_t empty = 0;
    for (size_t i = 0; i < cnt; ++i) empty += recs[i].dist == FZ_REC_NONE;
    if (!empty) return false;
    kept.clear();
    kept.reserve(cnt - empty);
    for (size_t i = 0; i < cnt; ++i) if (recs[i].dist != FZ_REC_NONE) kept.push_back(recs[i]);
    return true;
}

// idx_bound / blk_bound (0: unknown): every hit index is below idx_bound and every block number below blk_bound
// (sequence length and block count of the search) — saves the pass that finds the key ranges; may_have_empty: some
// records may be empty slots (the slot-per-hit verification).
// `into` (optional): the rows go into this vector instead of a result buffer (per-shard ordering of a sharded search).
int emit_matches(const FzRec *recs, size_t cnt, uint32_t L, fz_match **out, uint64_t *n, uint64_t idx_bound = 0,
                 uint32_t blk_bound = 0, bool may_have_empty = true, std::vector<fz_match> *into = nullptr) {
    size_t nv = 0;
    uint64_t imin = ~0ull, imax = 0;
    uint32_t gmax = 0;
    // key ranges known from the search (sequence length, number of blocks): no pass over the records for them — the
    // records sit in pinned memory the device has just written, and the first pass over them is the cold one; empty
    // slots (slot-per-hit kernels) are then dropped while the key words are built
    const bool bounds_known = idx_bound && blk_bound;
    if (bounds_known) {
        nv = cnt; imin = 0; imax = idx_bound - 1; gmax = blk_bound - 1;
    } else {
        // one pass for the empty slots (slot-per-hit kernels) and the key ranges
        for (size_t i = 0; i < cnt; ++i) {
            if (recs[i].dist == FZ_REC_NONE) continue;
            const uint64_t idx = fz_hit_index(recs[i].key);
            imin = std::min(imin, idx); imax = std::max(imax, idx);
            gmax = std::max(gmax, fz_hit_block(recs[i].key));
            ++nv;
        }
    }
    fz_match *mo = nullptr;
    auto make_room = [&]() -> int {                            // nv is final
        if (into) {
            into->resize(nv);
            mo = into->data();
            return FZ_OK;
        }
        void *mem = nullptr;
        int rc = alloc_out(nv, sizeof(fz_match), &mem);
        if (rc) return rc;
        mo = static_cast<fz_match *>(mem);
        *out = mo;
        *n = nv;
        return FZ_OK;
    };
    const bool count_later = bounds_known && may_have_empty && cnt > 0;   // nv = cnt is an upper bound until the key pass
    if (!count_later) { int rc = make_room(); if (rc) return rc; }
    auto put = [&](size_t i, const FzRec &r) {
        const uint64_t idx = fz_hit_index(r.key);
        mo[i].start = (int64_t)(idx - r.l);
        mo[i].end = (int64_t)(idx + L + r.r);
        mo[i].dist = (int32_t)r.dist;
        mo[i].block = (int32_t)fz_hit_block(r.key);
    };
    if (nv == 0) return count_later ? make_room() : FZ_OK;
    int ibits = 0, gbits = 0, pbits = 0;                       // index range, block number, record position
    while (ibits < FZ_IDX_BITS && ((imax - imin) >> ibits)) ++ibits;
    while ((gmax >> gbits)) ++gbits;
    while (((cnt - 1) >> pbits)) ++pbits;
    const int kbits = ibits + gbits;
    if (kbits + pbits <= 64) {
        // One 64-bit word per record: (block, index - imin) above the record's position.  ONE distribution pass on the
        // top digit of the key (about two buckets per record), then the buckets — a record or two each unless the
        // matches cluster — are put in order: sorting the whole words orders equal keys by position, and a search
        // never has two records with one key.  (2409 records: 14 -> ~7 us against three LSD passes with their own
        // range pass and two freshly allocated word arrays.)
        static thread_local std::vector<uint64_t> wa, wb;
        static thread_local std::vector<uint32_t> hist;
        if (wa.size() < nv) { wa.resize(nv + nv / 2 + 64); wb.resize(wa.size()); }
        int dbits = 1;                                         // about two records per bucket: the prefix sum and the bucket walk cost per bucket
        while (dbits < 16 && (2ull << dbits) < nv) ++dbits;
        dbits = std::max(1, std::min(dbits, std::max(1, kbits)));
        const int shift = pbits + kbits - dbits;
        const size_t nb = (size_t)1 << dbits;
        hist.assign(nb + 1, 0);
        uint64_t *a = wa.data(), *b = wb.data();
        size_t w = 0;
        for (size_t i = 0; i < cnt; ++i) {
            if (recs[i].dist == FZ_REC_NONE) continue;
            const uint64_t key = ((uint64_t)fz_hit_block(recs[i].key) << ibits) | (fz_hit_index(recs[i].key) - imin);
            const uint64_t word = (pbits < 64 ? key << pbits : 0) | (uint64_t)i;
            a[w++] = word;
            ++hist[(shift >= 0 ? (size_t)(word >> shift) : 0) + 1];
        }
        if (count_later) { nv = w; int rc = make_room(); if (rc) return rc; if (nv == 0) return FZ_OK; }
        for (size_t d = 0; d < nb; ++d) hist[d + 1] += hist[d];
        for (size_t i = 0; i < nv; ++i) b[hist[shift >= 0 ? (size_t)(a[i] >> shift) : 0]++] = a[i];
        // hist[d] is now the END of bucket d
        size_t s0 = 0;
        for (size_t d = 0; d < nb; ++d) {
            const size_t e0 = hist[d];
            const size_t len = e0 - s0;
            if (len > 24) std::sort(b + s0, b + e0);
            else if (len > 1) {
                for (size_t i = s0 + 1; i < e0; ++i) {
                    const uint64_t v = b[i];
                    size_t j = i;
                    while (j > s0 && b[j - 1] > v) { b[j] = b[j - 1]; --j; }
                    b[j] = v;
                }
            }
            s0 = e0;
        }
        const uint64_t pmask = pbits ? ((1ull << pbits) - 1) : 0;
        for (size_t i = 0; i < nv; ++i) put(i, recs[b[i] & pmask]);
        return FZ_OK;
    }
    std::vector<FzRec> copy;
    copy.reserve(nv);
    for (size_t i = 0; i < cnt; ++i) if (recs[i].dist != FZ_REC_NONE) copy.push_back(recs[i]);
    if (count_later) { nv = copy.size(); int rc = make_room(); if (rc) return rc; }
    sort_recs(copy);
    for (size_t i = 0; i < nv; ++i) put(i, copy[i]);
    return FZ_OK;
}

// Segmented searches (file API): reference order = segment (chunk) major, then (block, index).
int emit_matches_seg(const FzRec *recs, size_t cnt, uint32_t L, fz_match **out, uint64_t *n, uint32_t **seg_out) {
    std::vector<FzRec> kept;
    if (drop_empty_slots(recs, cnt, kept)) return emit_matches_seg(kept.data(), kept.size(), L, out, n, seg_out);
    void *mem = nullptr, *smem_ = nullptr;
    int rc = alloc_out(cnt, sizeof(fz_match), &mem);
    if (rc) return rc;
    rc = alloc_out(cnt, sizeof(uint32_t), &smem_);
    if (rc) { release_out(mem); return rc; }
    fz_match *mo = static_cast<fz_match *>(mem);
    uint32_t *so = static_cast<uint32_t *>(smem_);
    std::vector<uint32_t> order(cnt);
    for (size_t i = 0; i < cnt; ++i) order[i] = (uint32_t)i;
    std::sort(order.begin(), order.end(), [recs](uint32_t x, uint32_t y) {
        if (recs[x].aux != recs[y].aux) return recs[x].aux < recs[y].aux;
        return recs[x].key < recs[y].key;
    });
    for (size_t i = 0; i < cnt; ++i) {
        const FzRec &r = recs[order[i]];
        const uint64_t idx = fz_hit_index(r.key);
        mo[i].start = (int64_t)(idx - r.l);
        mo[i].end = (int64_t)(idx + L + r.r);
        mo[i].dist = (int32_t)r.dist;
        mo[i].block = (int32_t)fz_hit_block(r.key);
        so[i] = r.aux;
    }
    *out = mo; *n = cnt; *seg_out = so;
    return FZ_OK;
}

// A sharded search (several devices, or the ranks of an all-gather): every shard's records are ordered on their own —
// 10^4 records stay in the host's L2, one 8 x 10^4-record ordering does not (0.8 ms on 77 000 records) — and, shards
// owning ascending index ranges (seg_order lists them that way), the reference's order is, block by block, the shards'
// runs of that block one after the other.  merge_rows does the second half on rows that are already ordered.
int merge_rows(const std::vector<const std::vector<fz_match> *> &rows, const std::vector<uint32_t> &seg_order, fz_match **out, uint64_t *n) {
    const size_t ns = rows.size();
    size_t total = 0;
    for (size_t si = 0; si < ns; ++si) total += rows[si]->size();
    void *mem = nullptr;
    int rc = alloc_out(total, sizeof(fz_match), &mem);
    if (rc) return rc;
    fz_match *mo = static_cast<fz_match *>(mem);
    std::vector<size_t> pos(ns, 0);
    size_t o = 0;
    while (o < total) {
        int32_t g = INT32_MAX;                             // the smallest block any shard still holds
        for (size_t k = 0; k < ns; ++k) {
            const size_t si = seg_order[k];
            if (pos[si] < rows[si]->size()) g = std::min(g, (*rows[si])[pos[si]].block);
        }
        for (size_t k = 0; k < ns; ++k) {
            const size_t si = seg_order[k];
            const std::vector<fz_match> &r = *rows[si];
            size_t q = pos[si];
            // (a run of one block: gallop, then binary search — a shard holds thousands of rows per block)
            if (q < r.size() && r[q].block == g) {
                size_t step = 1, hi = q + 1;
                while (hi < r.size() && r[hi].block == g) { q = hi; hi = std::min(r.size(), hi + step); step <<= 1; }
                // r[q].block == g, and (hi == r.size() or r[hi].block != g): the run ends in (q, hi]
                size_t lo2 = q + 1, hi2 = hi;
                while (lo2 < hi2) { const size_t mid = (lo2 + hi2) / 2; if (r[mid].block == g) lo2 = mid + 1; else hi2 = mid; }
                q = lo2;
            }
            if (q > pos[si]) memcpy(mo + o, r.data() + pos[si], (q - pos[si]) * sizeof(fz_match));
            o += q - pos[si];
            pos[si] = q;
        }
    }
    *out = mo;
    *n = total;
    return FZ_OK;
}

// seg_ends[i] = end of shard i's records in `recs`.  With workers (ctx) the segments are ordered in parallel.
int emit_matches_segments(fz_ctx *ctx, const FzRec *recs, const std::vector<size_t> &seg_ends, const std::vector<uint32_t> &seg_order, uint32_t L,
                          fz_match **out, uint64_t *n, uint64_t idx_bound, uint32_t blk_bound, bool may_have_empty) {
    const size_t ns = seg_ends.size();
    static thread_local std::vector<std::vector<fz_match>> rows;
    if (rows.size() < ns) rows.resize(ns);
    std::vector<fz_match> *rowp = rows.data();
    auto order_one = [recs, &seg_ends, L, idx_bound, blk_bound, may_have_empty, rowp](size_t si) {
        const size_t b = si ? seg_ends[si - 1] : 0, e = seg_ends[si];
        return emit_matches(recs + b, e - b, L, nullptr, nullptr, idx_bound, blk_bound, may_have_empty, &rowp[si]);
    };
    if (ctx && ctx->workers && ns > 1 && ns <= ctx->workers->ws.size() && seg_ends.back() >= 4096) {
        for (size_t si = 0; si < ns; ++si) ctx->workers->post(si, [order_one, si]() { return order_one(si); });
        int rc = FZ_OK;
        for (size_t si = 0; si < ns; ++si) { const int r = ctx->workers->wait(si); if (r && !rc) rc = r; }
        if (rc) return rc;
    } else {
        for (size_t si = 0; si < ns; ++si) { int rc = order_one(si); if (rc) return rc; }
    }
    std::vector<const std::vector<fz_match> *> ptrs(ns);
    for (size_t si = 0; si < ns; ++si) ptrs[si] = &rows[si];
    return merge_rows(ptrs, seg_order, out, n);
}

// the records of the search that just ran: the staging-buffer view, the shards' ordered rows or the collected vector
int emit_matches(fz_ctx *ctx, const std::vector<FzRec> &recs, uint32_t L, fz_match **out, uint64_t *n,
                 uint64_t idx_bound = 0, uint32_t blk_bound = 0) {
    if (ctx->rows_ready) {                                 // several shards: ordered by search_collect, merged here
        std::vector<const std::vector<fz_match> *> ptrs(ctx->seg_order.size());
        for (size_t si = 0; si < ptrs.size(); ++si) ptrs[si] = &ctx->souts[si].rows;
        return merge_rows(ptrs, ctx->seg_order, out, n);
    }
    // (the fused scan appends real records only; the stand-alone verifications may leave empty slots)
    bool dense = true;
    for (const DevState &d : ctx->devs) dense = dense && d.cur().run.fused_used;
    if (!ctx->view && ctx->seg_ends.size() > 1 && ctx->seg_ends.back() == recs.size())
        return emit_matches_segments(ctx, recs.data(), ctx->seg_ends, ctx->seg_order, L, out, n, idx_bound, blk_bound, !dense);
    return ctx->view ? emit_matches(ctx->view, (size_t)ctx->view_n, L, out, n, idx_bound, blk_bound, !dense)
                     : emit_matches(recs.data(), recs.size(), L, out, n, idx_bound, blk_bound, !dense);
}

}  // namespace

extern "C" {

int fz_abi_version(void) { return FZ_ABI_VERSION; }

const char *fz_last_error(void) { return g_err.c_str(); }

int fz_device_count(int *n) {
    if (!n) return fail(FZ_EINVAL, "null argument");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; return fail(FZ_EDEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *n = c;
    return FZ_OK;
}

static int devstate_init(DevState &d) {
    HIP_TRY(hipSetDevice(d.device));
    // a search call is ~0.3 ms: spin instead of sleeping on the completion interrupt — on EVERY device of the context
    // (the flag is per device; refused with hipErrorSetOnActiveProcess once a device is in use: then it stays as it is)
    (void)hipSetDeviceFlags(hipDeviceScheduleSpin);
    (void)hipGetLastError();
    // Lowest priority: a different hardware queue than the default-priority streams of the rest of
    // the process, and the dispatcher prefers their workgroups.  Measured with RCCL on torch's
    // stream: at default priority an all_gather launched while a scan was running only started
    // after it (250 us); the scan alone is not slower at low priority.
    int prio_least = 0, prio_greatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    HIP_TRY(hipStreamCreateWithPriority(&d.stream, hipStreamNonBlocking, prio_least));
    HIP_TRY(hipStreamCreateWithPriority(&d.stream_alt, hipStreamNonBlocking, prio_least));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d.d_hdr_alt), kHeaderBytes));
    HIP_TRY(hipMemset(d.d_hdr_alt, 0, kHeaderBytes));
    for (ResultSlot &s : d.slots) {
        for (auto &ev : s.ev) HIP_TRY(hipEventCreate(&ev));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&s.h_stage), kHeaderBytes + kHostRecs * sizeof(FzRec), hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&s.h_stage_dev), s.h_stage, 0));
    }
    int rc = ensure_hits(d, 1u << 20);
    if (rc == FZ_OK) rc = ensure_recs(d, 1u << 16);
    return rc;
}

static void devstate_destroy(DevState &d) {
    (void)hipSetDevice(d.device);
    if (d.stream) (void)hipStreamSynchronize(d.stream);
    if (d.stream_alt) { (void)hipStreamSynchronize(d.stream_alt); (void)hipStreamDestroy(d.stream_alt); }
    if (d.d_hdr_alt) (void)hipFree(d.d_hdr_alt);
    if (d.d_hits) (void)hipFree(d.d_hits);
    if (d.d_out) (void)hipFree(d.d_out);
    if (d.spare_alloc) (void)hipFree(d.spare_alloc);
    for (auto &ev : d.rec_ev) if (ev) (void)hipEventDestroy(ev);
    for (ResultSlot &s : d.slots) {
        if (s.h_stage) (void)hipHostFree(s.h_stage);
        for (auto &ev : s.ev) if (ev) (void)hipEventDestroy(ev);
    }
    if (d.h_big) (void)hipHostFree(d.h_big);
    if (d.d_cand) (void)hipFree(d.d_cand);
    if (d.d_pat) (void)hipFree(d.d_pat);
    for (uint8_t *mp : {d.d_mp_desc, d.d_mp_ctr, d.d_mp_hits, d.d_mp_recs, d.d_assign, d.d_assign_recs}) if (mp) (void)hipFree(mp);
    if (d.d_gen_order) (void)hipFree(d.d_gen_order);
    if (d.d_gen_rows) (void)hipFree(d.d_gen_rows);
    if (d.d_gen_dedup) (void)hipFree(d.d_gen_dedup);
    for (int i = 0; i < 2; ++i) if (d.stream_h[i]) (void)hipHostFree(d.stream_h[i]);
    if (d.stream_d) (void)hipFree(d.stream_d);
    if (d.stream) (void)hipStreamDestroy(d.stream);
}

// the second lane (generic searches in flight): created on first use, hit lists as large as lane 0's
static int ensure_lane2(fz_ctx *ctx) {
    if (ctx->devs2.size() != ctx->devs.size()) {
        // built aside and only installed once EVERY device initialised: a half-built lane (out of memory part-way) must
        // not be mistaken for a usable one by the next call
        std::vector<DevState> lane(ctx->devs.size());
        for (size_t i = 0; i < ctx->devs.size(); ++i) {
            lane[i].device = ctx->devs[i].device;
            lane[i].n_cus = ctx->devs[i].n_cus;
            int rc = devstate_init(lane[i]);
            if (rc) {
                const std::string keep = g_err;
                for (size_t j = 0; j <= i; ++j) devstate_destroy(lane[j]);
                g_err = keep;
                return rc;
            }
        }
        ctx->devs2.swap(lane);
    }
    for (size_t i = 0; i < ctx->devs.size(); ++i) {
        int rc = ensure_hits(ctx->devs2[i], ctx->devs[i].hit_cap);
        if (rc) return rc;
    }
    return FZ_OK;
}

int fz_create(const int *device_ids, int n_devices, fz_ctx **out) {
    if (!out) return fail(FZ_EINVAL, "null argument");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(FZ_EDEVICE, "no HIP device available (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    // a search call is ~0.3 ms: spin instead of sleeping on the completion interrupt (ignored if the
    // runtime was already initialised with other flags, e.g. by torch in a distributed job)
    (void)hipSetDeviceFlags(hipDeviceScheduleSpin);
    (void)hipGetLastError();
    std::vector<int> ids;
    if (!device_ids || n_devices <= 0) ids.push_back(0);
    else ids.assign(device_ids, device_ids + n_devices);
    fz_ctx *ctx = new (std::nothrow) fz_ctx();
    if (!ctx) return fail(FZ_ENOMEM, "out of memory");
    for (int id : ids) {
        if (id < 0 || id >= count) { fz_destroy(ctx); return fail(FZ_EINVAL, "device id %d out of range (have %d)", id, count); }
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, id) != hipSuccess) { fz_destroy(ctx); return fail(FZ_EDEVICE, "hipGetDeviceProperties failed"); }
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            fz_destroy(ctx);
            return fail(FZ_EDEVICE, "device %d is %s; libfzhip is built for gfx950 (MI355X) only", id, prop.gcnArchName);
        }
        ctx->devs.emplace_back();
        DevState &d = ctx->devs.back();
        d.device = id;
        d.n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        int rc = devstate_init(d);
        if (rc) { fz_destroy(ctx); return rc; }
    }
    // Overlapped pipelines by default where they were measured: one device state.  Several device states of one context
    // may share a GPU (FZ_DEVICES=0,0); each brings two low-priority streams, and a process gets 4 hardware queues by
    // default, so their streams would share queues and the overlap is not what was measured.  They keep one stream per
    // device unless fz_set_streams(ctx, 2) asks for more.
    ctx->streams = ctx->devs.size() == 1 ? 2 : 1;
    if (ctx->devs.size() > 1 && !sw().no_dev_threads) {
        ctx->workers = new (std::nothrow) DevWorkers(ctx->devs.size());
        if (!ctx->workers) { fz_destroy(ctx); return fail(FZ_ENOMEM, "out of memory"); }
    }
    *out = ctx;
    return FZ_OK;
}

void fz_destroy(fz_ctx *ctx) {
    if (!ctx) return;
    delete ctx->workers;
    ctx->workers = nullptr;
    // sequences the caller never released: their device memory goes with the context (their handles die with it)
    while (!ctx->live.empty()) {
        for (DevState &d : ctx->devs) { (void)hipSetDevice(d.device); if (d.stream) (void)hipStreamSynchronize(d.stream); }
        fz_seq_release(ctx->live.back());
    }
    comm_teardown(ctx);
    for (DevState &d : ctx->devs) devstate_destroy(d);
    for (DevState &d : ctx->devs2) devstate_destroy(d);
    delete ctx;
}

// A shard's buffer: FZ_PAD_FRONT zero bytes, the body rounded up to whole tiles with everything behind geom.buf_len zeroed,
// FZ_PAD_BACK zero bytes (the scan kernels rely on the guard bytes).  The body's bytes are the caller's to write, on d.stream.
static int alloc_one(fz_ctx *ctx, int dev_index, const FzGeom &geom, Shard &sh) {
    DevState &d = ctx->devs[dev_index];
    HIP_TRY(hipSetDevice(d.device));
    const uint64_t tiles = (geom.buf_len + FZ_TILE_BYTES - 1) / FZ_TILE_BYTES;
    const uint64_t body = std::max<uint64_t>(1, tiles) * FZ_TILE_BYTES;
    sh.dev = dev_index;
    sh.alloc_bytes = FZ_PAD_FRONT + body + FZ_PAD_BACK;
    sh.geom = geom;
    if (d.spare_alloc && d.spare_bytes >= sh.alloc_bytes && d.spare_bytes <= 4 * sh.alloc_bytes + (1u << 20)) {
        sh.d_alloc = d.spare_alloc;               // recycle (the stream orders the reuse)
        sh.alloc_bytes = d.spare_bytes;
        d.spare_alloc = nullptr;
        d.spare_bytes = 0;
    } else {
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sh.d_alloc), sh.alloc_bytes));
    }
    sh.d_buf = sh.d_alloc + FZ_PAD_FRONT;
    HIP_TRY(hipMemsetAsync(sh.d_alloc, 0, FZ_PAD_FRONT, d.stream));
    HIP_TRY(hipMemsetAsync(sh.d_buf + geom.buf_len, 0, sh.alloc_bytes - FZ_PAD_FRONT - geom.buf_len, d.stream));
    return FZ_OK;
}

static int upload_one(fz_ctx *ctx, int dev_index, const uint8_t *host_buf, const FzGeom &geom, Shard &sh) {
    int rc = alloc_one(ctx, dev_index, geom, sh);
    if (rc) return rc;
    DevState &d = ctx->devs[dev_index];
    if (geom.buf_len) HIP_TRY(hipMemcpyAsync(sh.d_buf, host_buf, geom.buf_len, hipMemcpyHostToDevice, d.stream));
    // grow the hit list with the sequence: n-gram hits on 4-letter text run at ~G * n / 4^L
    return ensure_hits(d, std::max<uint64_t>(1u << 20, geom.buf_len / 64));
}

int fz_seq_upload(fz_ctx *ctx, const uint8_t *host, uint64_t n, fz_seq **out) {
    if (!ctx || !out || (!host && n)) return fail(FZ_EINVAL, "null argument");
    if (n >= (1ull << FZ_IDX_BITS)) return fail(FZ_EUNSUPPORTED, "sequence too long");
    *out = nullptr;
    fz_seq *seq = new (std::nothrow) fz_seq();
    if (!seq) return fail(FZ_ENOMEM, "out of memory");
    seq->ctx = ctx;
    seq->n = n;
    const uint64_t R = ctx->devs.size();
    const uint64_t halo = 2 * (uint64_t)FZ_MAX_M_ANY + 2 * FZ_MAX_K_ANY + 64;   // >= m + k for every supported query
    for (uint64_t r = 0; r < R; ++r) {
        FzGeom g{};
        g.n = n;
        g.own_lo = n / R * r + std::min<uint64_t>(r, n % R);
        g.own_hi = n / R * (r + 1) + std::min<uint64_t>(r + 1, n % R);
        const uint64_t lo = g.own_lo > halo ? g.own_lo - halo : 0;
        const uint64_t hi = std::min<uint64_t>(n, g.own_hi + halo);
        g.buf_off = lo;
        g.buf_len = hi - lo;
        if (R > 1 && g.own_hi == g.own_lo) continue;   // nothing to own
        seq->shards.emplace_back();
        int rc = upload_one(ctx, (int)r, host + lo, g, seq->shards.back());
        if (rc) { fz_seq_release(seq); return rc; }
    }
    for (Shard &sh : seq->shards) {
        (void)hipSetDevice(ctx->devs[sh.dev].device);
        hipError_t e = hipStreamSynchronize(ctx->devs[sh.dev].stream);
        if (e != hipSuccess) { fz_seq_release(seq); return fail(FZ_EDEVICE, "upload failed: %s", hipGetErrorString(e)); }
    }
    ctx->live.push_back(seq);
    *out = seq;
    return FZ_OK;
}

int fz_seq_upload_shard(fz_ctx *ctx, const uint8_t *host_buf, uint64_t buf_len, uint64_t buf_global_off,
                        uint64_t own_lo, uint64_t own_hi, uint64_t global_n, fz_seq **out) {
    if (!ctx || !out || (!host_buf && buf_len)) return fail(FZ_EINVAL, "null argument");
    if (global_n >= (1ull << FZ_IDX_BITS)) return fail(FZ_EUNSUPPORTED, "sequence too long");
    if (buf_global_off + buf_len > global_n || own_lo > own_hi || own_hi > global_n)
        return fail(FZ_EINVAL, "shard ranges outside the global sequence");
    if (own_hi > own_lo && (own_lo < buf_global_off || own_hi > buf_global_off + buf_len))
        return fail(FZ_EINVAL, "owned range not inside the shard buffer");
    *out = nullptr;
    fz_seq *seq = new (std::nothrow) fz_seq();
    if (!seq) return fail(FZ_ENOMEM, "out of memory");
    seq->ctx = ctx;
    seq->n = global_n;
    FzGeom g{};
    g.n = global_n;
    g.buf_off = buf_global_off;
    g.buf_len = buf_len;
    g.own_lo = own_lo;
    g.own_hi = own_hi;
    seq->shards.emplace_back();
    int rc = upload_one(ctx, 0, host_buf, g, seq->shards.back());
    if (rc == FZ_OK) {
        hipError_t e = hipStreamSynchronize(ctx->devs[0].stream);
        if (e != hipSuccess) rc = fail(FZ_EDEVICE, "upload failed: %s", hipGetErrorString(e));
    }
    if (rc) { fz_seq_release(seq); return rc; }
    ctx->live.push_back(seq);
    *out = seq;
    return FZ_OK;
}

int fz_seq_new(fz_ctx *ctx, uint64_t global_n, fz_seq **out) {
    if (!ctx || !out) return fail(FZ_EINVAL, "null argument");
    *out = nullptr;
    if (global_n >= (1ull << FZ_IDX_BITS)) return fail(FZ_EUNSUPPORTED, "sequence too long");
    fz_seq *seq = new (std::nothrow) fz_seq();
    if (!seq) return fail(FZ_ENOMEM, "out of memory");
    seq->ctx = ctx;
    seq->n = global_n;
    ctx->live.push_back(seq);
    *out = seq;
    return FZ_OK;
}

int fz_seq_add_shard(fz_seq *seq, int dev_index, const uint8_t *host_buf, uint64_t buf_len, uint64_t buf_global_off,
                     uint64_t own_lo, uint64_t own_hi) {
    if (!seq || !seq->ctx || (!host_buf && buf_len)) return fail(FZ_EINVAL, "null argument");
    fz_ctx *ctx = seq->ctx;
    if (seq->is_batch) return fail(FZ_EINVAL, "a batch handle takes no shards");
    if (ctx->npend || ctx->stream_inflight) return fail(FZ_EINVAL, "a search of this context is in flight");
    if (dev_index < 0 || dev_index >= (int)ctx->devs.size()) return fail(FZ_EINVAL, "device index %d outside the context (%zu devices)", dev_index, ctx->devs.size());
    if (buf_global_off + buf_len > seq->n || own_lo > own_hi || own_hi > seq->n)
        return fail(FZ_EINVAL, "shard ranges outside the global sequence");
    if (own_hi > own_lo && (own_lo < buf_global_off || own_hi > buf_global_off + buf_len))
        return fail(FZ_EINVAL, "owned range not inside the shard buffer");
    for (const Shard &o : seq->shards) {
        if (o.dev == dev_index) return fail(FZ_EINVAL, "device %d already holds a shard of this sequence", dev_index);
        if (own_lo < o.geom.own_hi && o.geom.own_lo < own_hi) return fail(FZ_EINVAL, "owned ranges of two shards overlap");
    }
    FzGeom g{};
    g.n = seq->n;
    g.buf_off = buf_global_off;
    g.buf_len = buf_len;
    g.own_lo = own_lo;
    g.own_hi = own_hi;
    seq->shards.emplace_back();
    int rc = upload_one(ctx, dev_index, host_buf, g, seq->shards.back());
    if (rc == FZ_OK) {
        hipError_t e = hipStreamSynchronize(ctx->devs[dev_index].stream);     // host_buf is only borrowed for this call
        if (e != hipSuccess) rc = fail(FZ_EDEVICE, "upload failed: %s", hipGetErrorString(e));
    }
    if (rc) {
        Shard &sh = seq->shards.back();
        if (sh.d_alloc) { (void)hipSetDevice(ctx->devs[dev_index].device); (void)hipFree(sh.d_alloc); }
        seq->shards.pop_back();
    }
    return rc;
}

int fz_device_ms(fz_ctx *ctx, double *filter_ms, int cap) {
    if (!ctx || (!filter_ms && cap > 0)) return fail(FZ_EINVAL, "null argument");
    resolve_timing(ctx);
    for (int i = 0; i < cap && i < (int)ctx->devs.size(); ++i) filter_ms[i] = ctx->devs[i].last_filter_ms;
    return (int)ctx->devs.size();
}

uint64_t fz_seq_len(const fz_seq *seq) { return seq ? seq->n : 0; }

void fz_seq_release(fz_seq *seq) {
    if (!seq) return;
    if (seq->ctx) {
        auto &live = seq->ctx->live;
        live.erase(std::remove(live.begin(), live.end(), seq), live.end());
    }
    for (Shard &sh : seq->shards) {
        if (sh.d_alloc) {
            DevState &d = seq->ctx->devs[sh.dev];
            (void)hipSetDevice(d.device);
            if (sh.alloc_bytes <= (64u << 20) && (!d.spare_alloc || d.spare_bytes < sh.alloc_bytes)) {
                if (d.spare_alloc) (void)hipFree(d.spare_alloc);
                d.spare_alloc = sh.d_alloc;       // keep small buffers for the next upload
                d.spare_bytes = sh.alloc_bytes;
            } else {
                (void)hipFree(sh.d_alloc);
            }
        }
    }
    if (seq->ctx && (seq->d_ends_base || seq->d_first || seq->d_src_starts || seq->d_fa_rows)) {
        (void)hipSetDevice(seq->ctx->devs[0].device);
        for (void *p : {(void *)seq->d_ends_base, (void *)seq->d_first, (void *)seq->d_src_starts, (void *)seq->d_fa_rows})
            if (p) (void)hipFree(p);
    }
    delete seq;
}

// ---------------------------------------------------------------------------------------------
// Batch uploads.  fz_batch_upload, fz_batch_upload_records and fz_batch_upload_fasta share their admission
// (batch_upload_admit) and the builder of their handle (batch_make_handle); the two that split a text on the device also
// share one Ingest per call: the line table, the growing scan, the verdict words and the timing epilogue.

static int batch_single_device(fz_ctx *ctx, fz_seq *batch) {
    if (ctx->devs.size() != 1 || ctx->snapshot || comm_multi_process(ctx) || (batch && batch->is_batch && batch->shards.size() != 1))
        return fail(FZ_EUNSUPPORTED, "batches are searched by single-device, non-collective contexts");
    return FZ_OK;
}

// What every batch upload asks of its context: the searches' rule, and nothing in flight.
static int batch_upload_admit(fz_ctx *ctx) {
    if (int rc = batch_single_device(ctx, nullptr)) return rc;
    if (ctx->npend || ctx->stream_inflight) return fail(FZ_EINVAL, "a search of this context is in flight");
    return FZ_OK;
}

// The handle of every batch upload: `total` bytes, which fill(d_buf) enqueues on the device's stream, and the tables over
// them (fz_device.h: ragged segments).  The scanned length table (n_seqs + 1 entries, the first 0) comes either from the
// host (host_offs: it is uploaded) or from the device (d_table: the handle owns it from here on, the pointer is cleared,
// and ends[] is read back; *d2h_ms = the host's wait for it).  An empty batch keeps null tables.  Not yet in ctx->live.
static int batch_make_handle(fz_ctx *ctx, uint64_t n_seqs, uint64_t total, uint64_t longest, const uint64_t *host_offs,
                             uint64_t *&d_table, double *d2h_ms, fz_seq **out, const std::function<int(uint8_t *)> &fill) {
    static_assert(FZ_RAG_TILE_BITS == FZ_TILE_BITS, "first[] is indexed by the scan's tiles");
    DevState &d = ctx->devs[0];
    fz_seq *seq = new (std::nothrow) fz_seq();
    if (!seq) return fail(FZ_ENOMEM, "out of memory");
    seq->ctx = ctx;
    seq->n = total;
    seq->is_batch = true;
    seq->n_seqs = n_seqs;
    seq->max_seq_len = longest;
    FzGeom g{};
    g.n = total;
    g.buf_off = 0;
    g.buf_len = total;
    g.own_lo = 0;
    g.own_hi = total;
    seq->shards.emplace_back();
    int rc = alloc_one(ctx, 0, g, seq->shards.back());
    if (rc == FZ_OK) rc = fill(seq->shards.back().d_buf);
    // grow the hit list with the batch: n-gram hits on 4-letter text run at ~G * n / 4^L
    if (rc == FZ_OK) rc = ensure_hits(d, std::max<uint64_t>(1u << 20, total / 64));
    std::vector<uint32_t> first;
    if (rc == FZ_OK && n_seqs) {
        hipError_t e;
        if (host_offs) {
            seq->ends.assign(host_offs + 1, host_offs + 1 + n_seqs);
            e = hipMalloc(reinterpret_cast<void **>(&seq->d_ends_base), (n_seqs + 1) * sizeof(uint64_t));
            if (e == hipSuccess) e = hipMemcpyAsync(seq->d_ends_base, host_offs, (n_seqs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, d.stream);
        } else {
            const auto t0 = std::chrono::steady_clock::now();
            seq->ends.resize(n_seqs);
            e = hipMemcpyAsync(seq->ends.data(), d_table + 1, n_seqs * sizeof(uint64_t), hipMemcpyDeviceToHost, d.stream);
            if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
            *d2h_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            seq->d_ends_base = d_table;
            d_table = nullptr;
        }
        // per tile the first sequence that touches it
        const uint64_t ntiles = (total + FZ_TILE_BYTES - 1) / FZ_TILE_BYTES;
        if (e == hipSuccess) {
            first.resize(ntiles + 1);
            fz_ragged_first(seq->ends.data(), n_seqs, ntiles, first.data());
            e = hipMalloc(reinterpret_cast<void **>(&seq->d_first), first.size() * sizeof(uint32_t));
        }
        if (e == hipSuccess) e = hipMemcpyAsync(seq->d_first, first.data(), first.size() * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream);
        if (e != hipSuccess) {
            rc = fail(e == hipErrorOutOfMemory ? FZ_ENOMEM : FZ_EDEVICE, "batch tables: %s", hipGetErrorString(e));
        } else {
            FzGeom &sg = seq->shards.back().geom;
            sg.seg_org = reinterpret_cast<uint64_t>(seq->d_ends_base + 1);
            sg.seg_j0 = reinterpret_cast<uint64_t>(seq->d_first);
            sg.seg_j1 = n_seqs;
        }
    }
    if (rc == FZ_OK) {
        hipError_t e = hipStreamSynchronize(d.stream);    // the caller's bytes and the tables' host copies are only borrowed
        if (e != hipSuccess) rc = fail(FZ_EDEVICE, "upload failed: %s", hipGetErrorString(e));
    }
    if (rc) { fz_seq_release(seq); return rc; }
    *out = seq;
    return FZ_OK;
}

int fz_batch_upload(fz_ctx *ctx, const uint8_t *bytes, const uint64_t *offs, uint64_t n_seqs, fz_seq **out) {
    if (!ctx || !out || !offs) return fail(FZ_EINVAL, "null argument");
    *out = nullptr;
    if (n_seqs >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "more than 2^32 - 1 sequences in a batch");
    if (offs[0] != 0) return fail(FZ_EINVAL, "offs[0] must be 0");
    for (uint64_t j = 0; j < n_seqs; ++j)
        if (offs[j + 1] < offs[j]) return fail(FZ_EINVAL, "sequence offsets must not decrease");
    uint64_t longest = 0;
    for (uint64_t j = 0; j < n_seqs; ++j) longest = std::max(longest, offs[j + 1] - offs[j]);
    const uint64_t n = offs[n_seqs];
    if (!bytes && n) return fail(FZ_EINVAL, "null argument");
    if (n >= (1ull << FZ_IDX_BITS)) return fail(FZ_EUNSUPPORTED, "sequence too long");
    int rc = batch_upload_admit(ctx);
    if (rc) return rc;
    // offs[] is the scanned length table that the text uploads make on the device: it goes up as it is
    fz_seq *seq = nullptr;
    uint64_t *no_table = nullptr;
    rc = batch_make_handle(ctx, n_seqs, n, longest, offs, no_table, nullptr, &seq, [&](uint8_t *d_buf) {
        if (n) HIP_TRY(hipMemcpyAsync(d_buf, bytes, n, hipMemcpyHostToDevice, ctx->devs[0].stream));
        return FZ_OK;
    });
    if (rc) return rc;
    ctx->live.push_back(seq);
    *out = seq;
    return FZ_OK;
}

int fz_debug_batch_segment(const uint64_t *offs, uint64_t n_seqs, uint64_t idx, uint64_t *j, uint64_t *sa, uint64_t *se) {
    if (!offs || !j || !sa || !se) return fail(FZ_EINVAL, "null argument");
    if (n_seqs >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "more than 2^32 - 1 sequences in a batch");
    const uint64_t n = offs[n_seqs];
    if (idx >= n) return fail(FZ_EINVAL, "position outside the batch");
    // the per-tile table of the offset array the last call named, kept while the caller keeps asking about that array
    static thread_local const uint64_t *c_offs = nullptr;
    static thread_local uint64_t c_nseqs = 0, c_n = 0;
    static thread_local std::vector<uint32_t> c_first;
    if (c_offs != offs || c_nseqs != n_seqs || c_n != n || c_first.empty()) {
        const uint64_t ntiles = (n + FZ_TILE_BYTES - 1) / FZ_TILE_BYTES;
        c_first.resize(ntiles + 1);
        fz_ragged_first(offs + 1, n_seqs, ntiles, c_first.data());
        c_offs = offs; c_nseqs = n_seqs; c_n = n;
    }
    FzRagged t;
    t.ends = offs + 1; t.first = c_first.data(); t.n_seqs = n_seqs;
    const FzSeg sg = fz_segment_ragged(t, n, idx);
    if (!sg.ok) return fail(FZ_EINVAL, "position outside the batch");
    *j = sg.j; *sa = sg.sa; *se = sg.se;
    return FZ_OK;
}

// ---------------------------------------------------------------------------------------------
// Records (fz_batch_upload_records): the text crosses PCIe once and is split where it lies (fz_kernels.h: fz_rec_*_kernel).
// What it shares with fz_batch_upload_fasta is here too: the reasons and their report, the scan, Ingest, the twins' helpers.

namespace {
const char *rec_reason_text(uint32_t reason) {
    switch (reason) {
    case FZ_REC_E_COUNT: return "the number of lines is not a multiple of 4 (truncated record)";
    case FZ_REC_E_AT: return "the header line does not start with '@'";
    case FZ_REC_E_PLUS: return "the separator line does not start with '+'";
    case FZ_REC_E_QUAL: return "the quality line is not as long as the sequence line";
    case FZ_FA_E_START: return "the text does not start with '>'";
    case FZ_FA_E_EMPTY: return "an empty line inside the sequence";
    case FZ_FA_E_WIDTH: return "the sequence lines are not of one length and width (all but the last, which may be shorter)";
    }
    return "malformed";
}

int rec_check_args(const uint8_t *text, uint64_t n, uint32_t period, uint32_t phase, uint32_t flags) {
    if (!text && n) return fail(FZ_EINVAL, "null argument");
    if (flags & ~FZ_REC_FASTQ_CHECKS) return fail(FZ_EINVAL, "unknown record flags");
    if (period == 0 || phase >= period) return fail(FZ_EINVAL, "sequence_line must be smaller than lines_per_record");
    if ((flags & FZ_REC_FASTQ_CHECKS) && (period != 4 || phase != 1)) return fail(FZ_EINVAL, "the FASTQ checks take 4 lines per record, the sequence on line 1");
    if (n >= (1ull << FZ_IDX_BITS)) return fail(FZ_EUNSUPPORTED, "sequence too long");
    return FZ_OK;
}

// FASTQ: trailing empty lines are no lines.  -> the length of the text without them.
uint64_t rec_trim(const uint8_t *text, uint64_t n) {
    for (;;) {
        if (n == 0) return 0;
        if (text[n - 1] == '\n') {
            if (n == 1 || text[n - 2] == '\n') { n -= 1; continue; }
            if (text[n - 2] == '\r' && (n == 2 || text[n - 3] == '\n')) { n -= 2; continue; }
            return n;
        }
        if (text[n - 1] == '\r' && (n == 1 || text[n - 2] == '\n')) { n -= 1; continue; }
        return n;
    }
}

int rec_report(const char *what, uint64_t key, fz_records_info *info) {
    if (info) { info->bad_record = fz_rec_err_record(key); info->bad_reason = fz_rec_err_reason(key); }
    return fail(FZ_EINVAL, "%s: record %llu: %s", what, (unsigned long long)fz_rec_err_record(key), rec_reason_text(fz_rec_err_reason(key)));
}

uint32_t rec_grid(const DevState &d, uint64_t items) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(items, (uint64_t)d.n_cus * 8)); }

// Exclusive scan of data[0 .. n) in place on d.stream; scratch holds rec_scan_scratch(n) u64.
uint64_t rec_scan_scratch(uint64_t n) {
    uint64_t blocks[FZ_RSCAN_MAX_LEVELS], total = 0;
    const int levels = fz_rscan_levels(n, blocks);
    for (int l = 0; l < levels; ++l) total += blocks[l];
    return total;
}

void rec_scan(DevState &d, uint64_t *data, uint64_t n, uint64_t *scratch) {
    uint64_t blocks[FZ_RSCAN_MAX_LEVELS];
    const int levels = fz_rscan_levels(n, blocks);
    uint64_t *at[FZ_RSCAN_MAX_LEVELS + 1];
    uint64_t cnt[FZ_RSCAN_MAX_LEVELS + 1];
    at[0] = data; cnt[0] = n;
    for (int l = 0; l < levels; ++l) { at[l + 1] = l ? at[l] + blocks[l - 1] : scratch; cnt[l + 1] = blocks[l]; }
    for (int l = 0; l < levels; ++l)                      // up: every level's workgroup sums
        hipLaunchKernelGGL(fz_rec_scan_reduce_kernel, dim3(rec_grid(d, cnt[l + 1])), dim3(FZ_RSCAN_THREADS), 0, d.stream, at[l], cnt[l], at[l + 1]);
    for (int l = levels; l >= 0; --l)                     // down: the top level is one workgroup
        hipLaunchKernelGGL(fz_rec_scan_down_kernel, dim3(rec_grid(d, (cnt[l] + FZ_RSCAN_ITEMS - 1) / FZ_RSCAN_ITEMS)), dim3(FZ_RSCAN_THREADS), 0,
                           d.stream, at[l], cnt[l], l < levels ? at[l + 1] : (uint64_t *)nullptr);
}

int rec_malloc_bytes(void **p, uint64_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) { *p = nullptr; return fail(e == hipErrorOutOfMemory ? FZ_ENOMEM : FZ_EDEVICE, "records: %s", hipGetErrorString(e)); }
    return FZ_OK;
}
#define rec_malloc(pp, count) rec_malloc_bytes(reinterpret_cast<void **>(pp), std::max<uint64_t>(1, (count)) * sizeof(**(pp)))

// One call of fz_batch_upload_records or fz_batch_upload_fasta: the transient device memory (freed when the call ends), the
// scan scratch with its capacity, the timing marks and the steps that the two calls share.  what ("records" / "fasta")
// goes in front of the frame's own error texts.
struct Ingest {
    fz_ctx *ctx;
    DevState &d;
    const char *what;
    const bool timed;
    const std::chrono::steady_clock::time_point t_call = std::chrono::steady_clock::now();
    int marks = 0;                                        // events recorded so far: mark() takes the next one
    double d2h_ms = 0;
    uint64_t n = 0, ntiles = 0, scratch_items = 0;
    uint8_t *raw = nullptr;
    uint64_t *counts = nullptr, *scratch = nullptr, *nl = nullptr, *starts = nullptr, *at = nullptr, *rank = nullptr, *head = nullptr;
    FzFaRow *rows = nullptr;
    unsigned long long *info = nullptr;

    Ingest(fz_ctx *c, const char *w) : ctx(c), d(c->devs[0]), what(w), timed(c->timing) {}
    ~Ingest() {
        for (void *p : {(void *)raw, (void *)counts, (void *)scratch, (void *)nl, (void *)starts, (void *)at, (void *)rank, (void *)head,
                        (void *)rows, (void *)info})
            if (p) (void)hipFree(p);
    }

    void mark() {
        if (timed && marks < (int)(sizeof(d.rec_ev) / sizeof(d.rec_ev[0]))) (void)hipEventRecord(d.rec_ev[marks], d.stream);
        ++marks;
    }

    // The exclusive scan of data[0 .. items) in place, the scratch grown when this one needs more.
    int scan(uint64_t *data, uint64_t items) {
        if (rec_scan_scratch(items) > scratch_items) {
            if (scratch) (void)hipFree(scratch);
            scratch = nullptr;
            scratch_items = rec_scan_scratch(items);
            if (int rc = rec_malloc(&scratch, scratch_items)) return rc;
        }
        rec_scan(d, data, items, scratch);
        return FZ_OK;
    }

    // Stage 1 (marks 0 .. 3): the text in whole tiles (zeros behind it are no newlines), the newlines per tile, their
    // exclusive scan with the total behind it, the count read back, and nl[], every newline's position, enqueued.
    int line_table(const uint8_t *text, uint64_t n_, uint64_t *n_nl, uint64_t *n_lines) {
        n = n_;
        ntiles = (n + FZ_TILE_BYTES - 1) / FZ_TILE_BYTES;
        *n_nl = 0;
        HIP_TRY(hipSetDevice(d.device));
        if (timed) for (auto &ev : d.rec_ev) if (!ev) HIP_TRY(hipEventCreate(&ev));
        mark();
        if (n) {
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&raw), ntiles * FZ_TILE_BYTES));
            if (ntiles * FZ_TILE_BYTES > n) HIP_TRY(hipMemsetAsync(raw + n, 0, ntiles * FZ_TILE_BYTES - n, d.stream));
            HIP_TRY(hipMemcpyAsync(raw, text, n, hipMemcpyHostToDevice, d.stream));
        }
        mark();
        if (n) {
            if (int rc = rec_malloc(&counts, ntiles + 1)) return rc;
            HIP_TRY(hipMemsetAsync(counts + ntiles, 0, sizeof(uint64_t), d.stream));
            hipLaunchKernelGGL(fz_rec_count_kernel, dim3(rec_grid(d, ntiles)), dim3(FZ_REC_THREADS), 0, d.stream, raw, ntiles, counts);
            if (int rc = scan(counts, ntiles + 1)) return rc;
        }
        mark();
        if (n) {
            HIP_TRY(hipMemcpyAsync(n_nl, counts + ntiles, sizeof(uint64_t), hipMemcpyDeviceToHost, d.stream));
            HIP_TRY(hipStreamSynchronize(d.stream));
            if (*n_nl > n) return fail(FZ_EDEVICE, "%s: the newline count is outside the text", what);
        }
        *n_lines = fz_rec_n_lines(text, n, *n_nl);
        mark();                                           // the caller's kernels follow in this span, up to its next mark
        if (*n_lines) {
            if (int rc = rec_malloc(&nl, *n_nl)) return rc;
            if (*n_nl) hipLaunchKernelGGL(fz_rec_lines_kernel, dim3(rec_grid(d, ntiles)), dim3(FZ_REC_THREADS), 0, d.stream, raw, ntiles, counts, nl);
        }
        return FZ_OK;
    }

    // The verdict words of the measure and check kernels: info[0] = the smallest error key, info[1] = the longest sequence.
    int arm_verdict() {
        if (int rc = rec_malloc(&info, 2)) return rc;
        HIP_TRY(hipMemsetAsync(info, 0xff, sizeof(uint64_t), d.stream));
        HIP_TRY(hipMemsetAsync(info + 1, 0, sizeof(uint64_t), d.stream));
        return FZ_OK;
    }

    // ... read back with the packed length, the last entry of the scanned at[]; *key keeps the smaller of the caller's and
    // the kernels'.  A malformed record is reported before the lengths are doubted: the FASTA kernels measure a refused
    // text's records as they come.  For the records path the order makes no difference, since the lengths of the lines it
    // keeps never sum to more than n.
    int read_verdict(uint64_t n_seqs, uint64_t *key, uint64_t *total, uint64_t *longest) {
        unsigned long long got[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(got, info, sizeof(got), hipMemcpyDeviceToHost, d.stream));
        HIP_TRY(hipMemcpyAsync(total, at + n_seqs, sizeof(uint64_t), hipMemcpyDeviceToHost, d.stream));
        HIP_TRY(hipStreamSynchronize(d.stream));
        *key = std::min<uint64_t>(*key, got[0]);
        *longest = got[1];
        if (*key == FZ_REC_NO_ERROR && (*total > n || *longest > *total)) return fail(FZ_EDEVICE, "%s: the packed length is outside the text", what);
        return FZ_OK;
    }

    // The handle of fz_batch_upload over `total` bytes, which gather(d_buf) enqueues between two marks; at[] and starts[]
    // become the handle's.
    int handle(uint64_t n_seqs, uint64_t total, uint64_t longest, fz_seq **seq, const std::function<void(uint8_t *)> &gather) {
        int rc = batch_make_handle(ctx, n_seqs, total, longest, nullptr, at, &d2h_ms, seq, [&](uint8_t *d_buf) {
            mark();
            if (total) gather(d_buf);
            mark();
            return FZ_OK;
        });
        if (rc == FZ_OK && n_seqs) { (*seq)->d_src_starts = starts; starts = nullptr; }
        return rc;
    }

    // The last step: the spans of the marks go to rec_ms[] (the copy is (0, 1), the kernels are every (i, i + 1) of an odd
    // i), and the handle is the caller's.
    int finish(fz_seq *seq, fz_seq **out) {
        if (timed) {
            ctx->rec_ms[0] = span_ms(d.rec_ev[0], d.rec_ev[1]);
            ctx->rec_ms[1] = 0;
            for (int i = 1; i + 1 < marks; i += 2) ctx->rec_ms[1] += span_ms(d.rec_ev[i], d.rec_ev[i + 1]);
            ctx->rec_ms[2] = d2h_ms;
        }
        ctx->rec_ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
        ctx->live.push_back(seq);
        *out = seq;
        return FZ_OK;
    }
};

// The twins on the host (fz_debug_records_split, fz_debug_fasta_split): every newline's position, by the kernels' byte mask
// word by word ...
void host_line_table(const uint8_t *text, uint64_t n, std::vector<uint64_t> &nl) {
    uint64_t i = 0;
    for (; i + 4 <= n; i += 4) {
        uint32_t w;
        memcpy(&w, text + i, 4);
        for (uint32_t m = fz_rec_nl_mask(w); m; m &= m - 1u) nl.push_back(i + ((uint32_t)__builtin_ctz(m) >> 3));
    }
    for (; i < n; ++i) if (text[i] == '\n') nl.push_back(i);
}

// ... and the three arrays they hand out: n_seqs rows of `row` bytes, n_seqs ends, the packed bytes.  All or none.
int alloc_split_out(uint64_t n_seqs, size_t row, uint64_t packed, void **rows, void **ends, void **bytes) {
    int rc = alloc_out(n_seqs, row, rows);
    if (rc == FZ_OK) rc = alloc_out(n_seqs, sizeof(uint64_t), ends);
    if (rc == FZ_OK) rc = alloc_out(packed, 1, bytes);
    if (rc) { release_out(*rows); release_out(*ends); release_out(*bytes); *rows = *ends = *bytes = nullptr; }
    return rc;
}

}  // namespace

int fz_batch_upload_records(fz_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t lines_per_record, uint32_t sequence_line,
                            uint32_t flags, fz_seq **out, fz_records_info *info) {
    if (!ctx || !out) return fail(FZ_EINVAL, "null argument");
    *out = nullptr;
    if (info) *info = fz_records_info{};
    int rc = rec_check_args(text, n, lines_per_record, sequence_line, flags);
    if (rc == FZ_OK) rc = batch_upload_admit(ctx);
    if (rc) return rc;
    Ingest in(ctx, "records");
    DevState &d = in.d;
    if (flags & FZ_REC_FASTQ_CHECKS) n = rec_trim(text, n);
    // 1. the line table (a text with newlines and no whole record gets it too, before it is refused or comes out empty)
    uint64_t n_nl = 0, n_lines = 0;
    if ((rc = in.line_table(text, n, &n_nl, &n_lines))) return rc;
    const uint64_t n_seqs = fz_rec_n_seqs(n_lines, lines_per_record, sequence_line);
    if (info) { info->n_lines = n_lines; info->n_seqs = n_seqs; }
    if (n_seqs >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "more than 2^32 - 1 sequences in a batch");
    // 2. one lane per record; the scan of the lengths
    uint64_t key = fz_rec_count_key(n_lines, lines_per_record, flags), total = 0, longest = 0;
    if (n_seqs) {
        if ((rc = rec_malloc(&in.starts, n_seqs))) return rc;
        if ((rc = rec_malloc(&in.at, n_seqs + 1))) return rc;
        if ((rc = in.arm_verdict())) return rc;
        hipLaunchKernelGGL(fz_rec_measure_kernel, dim3(rec_grid(d, (n_seqs + FZ_REC_THREADS - 1) / FZ_REC_THREADS)), dim3(FZ_REC_THREADS), 0, d.stream,
                           in.raw, n, in.nl, n_nl, n_lines, lines_per_record, sequence_line, flags, n_seqs, in.starts, in.at, in.info);
        if ((rc = in.scan(in.at, n_seqs + 1))) return rc;
    }
    in.mark();
    if (n_seqs && (rc = in.read_verdict(n_seqs, &key, &total, &longest))) return rc;
    if (key != FZ_REC_NO_ERROR) return rec_report((flags & FZ_REC_FASTQ_CHECKS) ? "fastq" : "lines", key, info);
    if (info) info->packed_bytes = total;
    // 3. the handle, its bytes gathered on the device
    fz_seq *seq = nullptr;
    rc = in.handle(n_seqs, total, longest, &seq, [&](uint8_t *d_buf) {
        hipLaunchKernelGGL(fz_rec_gather_kernel, dim3(rec_grid(d, (total + FZ_TILE_BYTES - 1) / FZ_TILE_BYTES)), dim3(FZ_REC_THREADS), 0, d.stream,
                           in.raw, in.starts, in.at, n_seqs, total, d_buf);
    });
    if (rc) return rc;
    return in.finish(seq, out);
}

int fz_debug_records_ms(fz_ctx *ctx, double *ms4) {
    if (!ctx || !ms4) return fail(FZ_EINVAL, "null argument");
    for (int i = 0; i < 4; ++i) ms4[i] = ctx->rec_ms[i];
    return FZ_OK;
}

uint32_t fz_debug_scan_items(void) { return FZ_RSCAN_ITEMS; }

int fz_batch_tables(const fz_seq *batch, uint64_t *src_starts, uint64_t *ends) {
    if (!batch) return fail(FZ_EINVAL, "null argument");
    if (!batch->is_batch) return fail(FZ_EINVAL, "fz_batch_tables takes a batch handle");
    const uint64_t ns = batch->n_seqs;
    if (ends && ns) memcpy(ends, batch->ends.data(), ns * sizeof(uint64_t));
    if (src_starts && ns) {
        if (batch->d_src_starts) {
            HIP_TRY(hipSetDevice(batch->ctx->devs[0].device));
            HIP_TRY(hipMemcpy(src_starts, batch->d_src_starts, ns * sizeof(uint64_t), hipMemcpyDeviceToHost));
        } else {
            src_starts[0] = 0;
            for (uint64_t j = 1; j < ns; ++j) src_starts[j] = batch->ends[j - 1];
        }
    }
    return FZ_OK;
}

int fz_debug_batch_bytes(fz_seq *batch, uint8_t *out, uint64_t cap) {
    if (!batch || (!out && cap)) return fail(FZ_EINVAL, "null argument");
    if (!batch->is_batch || batch->shards.size() != 1) return fail(FZ_EINVAL, "fz_debug_batch_bytes takes a batch handle");
    if (cap < batch->n) return fail(FZ_EINVAL, "the buffer is smaller than the batch");
    if (batch->n == 0) return FZ_OK;
    const Shard &sh = batch->shards[0];
    DevState &d = batch->ctx->devs[sh.dev];
    HIP_TRY(hipSetDevice(d.device));
    HIP_TRY(hipMemcpyAsync(out, sh.d_buf, batch->n, hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    return FZ_OK;
}

int fz_debug_records_split(const uint8_t *text, uint64_t n, uint32_t lines_per_record, uint32_t sequence_line, uint32_t flags,
                           uint64_t **src_starts, uint64_t **ends, uint8_t **packed, fz_records_info *info) {
    if (!src_starts || !ends || !packed) return fail(FZ_EINVAL, "null argument");
    *src_starts = nullptr; *ends = nullptr; *packed = nullptr;
    if (info) *info = fz_records_info{};
    int rc = rec_check_args(text, n, lines_per_record, sequence_line, flags);
    if (rc) return rc;
    if (flags & FZ_REC_FASTQ_CHECKS) n = rec_trim(text, n);
    std::vector<uint64_t> nl;
    host_line_table(text, n, nl);
    const uint64_t n_nl = nl.size();
    const uint64_t n_lines = fz_rec_n_lines(text, n, n_nl);
    const uint64_t n_seqs = fz_rec_n_seqs(n_lines, lines_per_record, sequence_line);
    if (info) { info->n_lines = n_lines; info->n_seqs = n_seqs; }
    if (n_seqs >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "more than 2^32 - 1 sequences in a batch");
    uint64_t key = fz_rec_count_key(n_lines, lines_per_record, flags), total = 0;
    std::vector<FzRecOut> recs(n_seqs);
    for (uint64_t r = 0; r < n_seqs; ++r) {
        recs[r] = fz_rec_measure(text, n, nl.data(), n_nl, n_lines, lines_per_record, sequence_line, flags, r);
        if (recs[r].reason != FZ_REC_OK) key = std::min(key, fz_rec_err_key(r, recs[r].reason));
        total += recs[r].len;
    }
    if (key != FZ_REC_NO_ERROR) return rec_report((flags & FZ_REC_FASTQ_CHECKS) ? "fastq" : "lines", key, info);
    if (info) info->packed_bytes = total;
    void *ms = nullptr, *me = nullptr, *mp = nullptr;
    if ((rc = alloc_split_out(n_seqs, sizeof(uint64_t), total, &ms, &me, &mp))) return rc;
    uint64_t at = 0;
    for (uint64_t r = 0; r < n_seqs; ++r) {
        static_cast<uint64_t *>(ms)[r] = recs[r].start;
        if (recs[r].len) memcpy(static_cast<uint8_t *>(mp) + at, text + recs[r].start, recs[r].len);
        at += recs[r].len;
        static_cast<uint64_t *>(me)[r] = at;
    }
    *src_starts = static_cast<uint64_t *>(ms); *ends = static_cast<uint64_t *>(me); *packed = static_cast<uint8_t *>(mp);
    return FZ_OK;
}

// ---------------------------------------------------------------------------------------------
// FASTA (fz_batch_upload_fasta): the records path's line table, then headers ranked, records measured, lines checked and
// the bases gathered without their newlines (fz_kernels.h: fz_fa_*_kernel; the rule: fz_device.h).

namespace {
static_assert(sizeof(FzFaRow) == sizeof(fz_fasta_row) && sizeof(fz_fasta_row) == 48, "fz_fasta_row is FzFaRow");

int fa_check_args(const uint8_t *text, uint64_t n, uint32_t flags) {
    if (!text && n) return fail(FZ_EINVAL, "null argument");
    if (flags & ~FZ_FA_UPPER) return fail(FZ_EINVAL, "unknown fasta flags");
    if (n >= (1ull << FZ_IDX_BITS)) return fail(FZ_EUNSUPPORTED, "sequence too long");
    return FZ_OK;
}

}  // namespace

int fz_batch_upload_fasta(fz_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t flags, fz_seq **out, fz_records_info *info) {
    if (!ctx || !out) return fail(FZ_EINVAL, "null argument");
    *out = nullptr;
    if (info) *info = fz_records_info{};
    int rc = fa_check_args(text, n, flags);
    if (rc == FZ_OK) rc = batch_upload_admit(ctx);
    if (rc) return rc;
    Ingest in(ctx, "fasta");
    DevState &d = in.d;
    n = rec_trim(text, n);
    // 1. the line table
    uint64_t n_nl = 0, n_lines = 0, n_seqs = 0;
    if ((rc = in.line_table(text, n, &n_nl, &n_lines))) return rc;
    // 2. one lane per line flags the headers; the scan of the flags ranks every line into its record
    if (n_lines) {
        if ((rc = rec_malloc(&in.rank, n_lines + 1))) return rc;
        hipLaunchKernelGGL(fz_fa_heads_kernel, dim3(rec_grid(d, n_lines / FZ_REC_THREADS + 1)), dim3(FZ_REC_THREADS), 0, d.stream, in.raw, in.nl,
                           n_lines, in.rank, (uint64_t *)nullptr);
        if ((rc = in.scan(in.rank, n_lines + 1))) return rc;
    }
    in.mark();
    if (n_lines) {
        HIP_TRY(hipMemcpyAsync(&n_seqs, in.rank + n_lines, sizeof(uint64_t), hipMemcpyDeviceToHost, d.stream));
        HIP_TRY(hipStreamSynchronize(d.stream));
        if (n_seqs > n_lines) return fail(FZ_EDEVICE, "fasta: the header count is outside the text");
    }
    if (info) { info->n_lines = n_lines; info->n_seqs = n_seqs; }
    if (n_seqs >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "more than 2^32 - 1 sequences in a batch");
    // 3. every header's line; one lane per record; one lane per line; the scan of the lengths
    uint64_t key = fz_fa_text_key(text, n), total = 0, longest = 0;
    in.mark();
    if (n_seqs) {
        if ((rc = rec_malloc(&in.head, n_seqs + 1))) return rc;
        if ((rc = rec_malloc(&in.rows, n_seqs))) return rc;
        if ((rc = rec_malloc(&in.starts, n_seqs))) return rc;
        if ((rc = rec_malloc(&in.at, n_seqs + 1))) return rc;
        if ((rc = in.arm_verdict())) return rc;
        hipLaunchKernelGGL(fz_fa_heads_kernel, dim3(rec_grid(d, n_lines / FZ_REC_THREADS + 1)), dim3(FZ_REC_THREADS), 0, d.stream, in.raw, in.nl,
                           n_lines, in.rank, in.head);
        hipLaunchKernelGGL(fz_fa_measure_kernel, dim3(rec_grid(d, (n_seqs + FZ_REC_THREADS - 1) / FZ_REC_THREADS)), dim3(FZ_REC_THREADS), 0, d.stream,
                           in.raw, n, in.nl, n_nl, in.head, n_seqs, in.rows, in.starts, in.at, in.info);
        hipLaunchKernelGGL(fz_fa_check_kernel, dim3(rec_grid(d, (n_lines + FZ_REC_THREADS - 1) / FZ_REC_THREADS)), dim3(FZ_REC_THREADS), 0, d.stream,
                           in.raw, n, in.nl, n_nl, n_lines, in.rank, in.head, in.rows, in.info);
        if ((rc = in.scan(in.at, n_seqs + 1))) return rc;
    }
    in.mark();
    if (n_seqs && (rc = in.read_verdict(n_seqs, &key, &total, &longest))) return rc;
    if (key != FZ_REC_NO_ERROR) return rec_report("fasta", key, info);
    if (info) info->packed_bytes = total;
    // 4. the handle, its bases gathered on the device; the index rows stay with it
    fz_seq *seq = nullptr;
    rc = in.handle(n_seqs, total, longest, &seq, [&](uint8_t *d_buf) {
        hipLaunchKernelGGL(fz_fa_gather_kernel, dim3(rec_grid(d, (total + FZ_TILE_BYTES - 1) / FZ_TILE_BYTES)), dim3(FZ_REC_THREADS), 0, d.stream,
                           in.raw, in.rows, in.at, n_seqs, total, flags, d_buf);
    });
    if (rc) return rc;
    seq->d_fa_rows = in.rows;
    in.rows = nullptr;
    seq->is_fasta = true;
    return in.finish(seq, out);
}

int fz_batch_fasta_index(const fz_seq *batch, fz_fasta_row *rows) {
    if (!batch || !rows) return fail(FZ_EINVAL, "null argument");
    if (!batch->is_batch || !batch->is_fasta) return fail(FZ_EINVAL, "fz_batch_fasta_index takes a handle of fz_batch_upload_fasta");
    if (batch->n_seqs == 0) return FZ_OK;
    HIP_TRY(hipSetDevice(batch->ctx->devs[0].device));
    HIP_TRY(hipMemcpy(rows, batch->d_fa_rows, batch->n_seqs * sizeof(fz_fasta_row), hipMemcpyDeviceToHost));
    return FZ_OK;
}

int fz_debug_fasta_split(const uint8_t *text, uint64_t n, uint32_t flags, fz_fasta_row **rows, uint64_t **ends, uint8_t **packed,
                         fz_records_info *info) {
    if (!rows || !ends || !packed) return fail(FZ_EINVAL, "null argument");
    *rows = nullptr; *ends = nullptr; *packed = nullptr;
    if (info) *info = fz_records_info{};
    int rc = fa_check_args(text, n, flags);
    if (rc) return rc;
    n = rec_trim(text, n);
    std::vector<uint64_t> nl;
    host_line_table(text, n, nl);
    const uint64_t n_nl = nl.size();
    const uint64_t n_lines = fz_rec_n_lines(text, n, n_nl);
    std::vector<uint64_t> rank(n_lines + 1), head;       // the kernels' tables: the scanned flags, every header's line
    uint64_t n_seqs = 0;
    for (uint64_t i = 0; i < n_lines; ++i) {
        rank[i] = n_seqs;
        if (fz_fa_is_head(text, nl.data(), i)) { head.push_back(i); ++n_seqs; }
    }
    rank[n_lines] = n_seqs;
    head.push_back(n_lines);
    if (info) { info->n_lines = n_lines; info->n_seqs = n_seqs; }
    if (n_seqs >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "more than 2^32 - 1 sequences in a batch");
    uint64_t key = fz_fa_text_key(text, n), total = 0;
    std::vector<FzFaRow> recs(n_seqs);
    for (uint64_t r = 0; r < n_seqs; ++r) {
        const FzFaOut o = fz_fa_measure(text, n, nl.data(), n_nl, head.data(), r);
        recs[r] = o.row;
        if (o.reason != FZ_REC_OK) key = std::min(key, fz_rec_err_key(r, o.reason));
        total += o.row.length;
    }
    for (uint64_t i = 0; i < n_lines; ++i) {
        const uint64_t c = rank[i + 1];
        if (c == 0 || head[c - 1] == i) continue;
        const uint32_t why = fz_fa_line_check(text, n, nl.data(), n_nl, i, i + 1 == head[c], recs[c - 1].linebases, recs[c - 1].linewidth);
        if (why != FZ_REC_OK) key = std::min(key, fz_rec_err_key(c - 1, why));
    }
    if (key != FZ_REC_NO_ERROR) return rec_report("fasta", key, info);
    if (info) info->packed_bytes = total;
    void *mr = nullptr, *me = nullptr, *mp = nullptr;
    if ((rc = alloc_split_out(n_seqs, sizeof(fz_fasta_row), (total + 3) / 4 * 4, &mr, &me, &mp))) return rc;
    uint8_t *dst = static_cast<uint8_t *>(mp);
    uint64_t at = 0;
    for (uint64_t r = 0; r < n_seqs; ++r) {
        memcpy(static_cast<fz_fasta_row *>(mr) + r, &recs[r], sizeof(fz_fasta_row));
        for (uint64_t q = 0; q < recs[r].length; ++q) dst[at + q] = text[fz_fa_src(recs[r].offset, recs[r].linebases, recs[r].linewidth, q)];
        at += recs[r].length;
        static_cast<uint64_t *>(me)[r] = at;
    }
    if (flags & FZ_FA_UPPER)                              // a dword at a time, as the gather folds (bytes behind `total`: the buffer's own)
        for (uint64_t i = 0; i < total; i += 4) {
            uint32_t w = 0;
            memcpy(&w, dst + i, 4);
            w = fz_fa_upper4(w);
            memcpy(dst + i, &w, 4);
        }
    *rows = static_cast<fz_fasta_row *>(mr); *ends = static_cast<uint64_t *>(me); *packed = dst;
    return FZ_OK;
}

uint32_t fz_debug_fasta_upper4(uint32_t w) { return fz_fa_upper4(w); }

uint64_t fz_debug_fasta_src(uint64_t offset, uint64_t linebases, uint64_t linewidth, uint64_t q) {
    return linebases ? fz_fa_src(offset, linebases, linewidth, q) : offset;
}

// ---------------------------------------------------------------------------------------------
// Derived batches (fz_batch_derive): a third producer for batch_make_handle, next to the two text uploads.  It uploads the
// caller's tables and no text: one lane per output measures and checks its cut of the parent (fz_kernels.h:
// fz_derive_measure_kernel), the records path's scan places the outputs, and the gather fills the new handle from the
// parent's packed bytes where they lie.

namespace {
static_assert(sizeof(fz_derive_info) == 40, "fz_derive_info");

const char *drv_reason_text(uint32_t reason) {
    switch (reason) {
    case FZ_DRV_E_INDEX: return "the index is not a sequence of the parent batch";
    case FZ_DRV_E_ORDER: return "the start lies behind the end";
    case FZ_DRV_E_END: return "the end lies behind the end of the parent sequence";
    }
    return "bad item";
}

int drv_report(uint64_t key, fz_derive_info *info) {
    if (info) { info->bad_item = fz_rec_err_record(key); info->bad_reason = fz_rec_err_reason(key); }
    return fail(FZ_EINVAL, "derive: item %llu: %s", (unsigned long long)fz_rec_err_record(key), drv_reason_text(fz_rec_err_reason(key)));
}

int drv_check_args(uint64_t n_src, bool has_index, uint64_t n_out, uint32_t flags) {
    if (flags & ~FZ_DERIVE_REVERSE) return fail(FZ_EINVAL, "unknown derive flags");
    if (n_out >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "more than 2^32 - 1 sequences in a batch");
    if (!has_index && n_out != n_src) return fail(FZ_EINVAL, "without an index the derived batch has the parent's number of sequences");
    return FZ_OK;
}

// The caller's tables on the device for the length of one call.
struct DrvTables {
    uint32_t *index = nullptr, *xlat = nullptr;
    uint64_t *starts = nullptr, *ends = nullptr;
    ~DrvTables() {
        for (void *p : {(void *)index, (void *)xlat, (void *)starts, (void *)ends})
            if (p) (void)hipFree(p);
    }
};

int drv_upload_bytes(DevState &d, void **dst, const void *src, uint64_t bytes) {
    if (!src || !bytes) return FZ_OK;
    if (int rc = rec_malloc_bytes(dst, bytes)) return rc;
    HIP_TRY(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, d.stream));
    return FZ_OK;
}
#define drv_upload(d, pp, src, count) drv_upload_bytes(d, reinterpret_cast<void **>(pp), src, (count) * sizeof(**(pp)))
}  // namespace

int fz_batch_derive(fz_ctx *ctx, fz_seq *batch, const uint32_t *index, const uint64_t *starts, const uint64_t *ends, uint64_t n_out,
                    uint32_t flags, const uint8_t *translate, fz_seq **out, fz_derive_info *info) {
    if (!ctx || !batch || !out) return fail(FZ_EINVAL, "null argument");
    *out = nullptr;
    if (info) *info = fz_derive_info{};
    int rc = batch_upload_admit(ctx);
    if (rc) return rc;
    if (std::find(ctx->live.begin(), ctx->live.end(), batch) == ctx->live.end())
        return fail(FZ_EINVAL, "fz_batch_derive takes a live batch handle of this context");
    if (!batch->is_batch) return fail(FZ_EINVAL, "fz_batch_derive takes a batch handle");
    if (batch->shards.size() != 1) return fail(FZ_EUNSUPPORTED, "batches are derived on one device");
    const uint64_t n_src = batch->n_seqs;
    if ((rc = drv_check_args(n_src, index != nullptr, n_out, flags))) return rc;
    if (info) info->n_out = n_out;
    Ingest in(ctx, "derive");
    DevState &d = in.d;
    DrvTables tb;
    HIP_TRY(hipSetDevice(d.device));
    if (in.timed) for (auto &ev : d.rec_ev) if (!ev) HIP_TRY(hipEventCreate(&ev));
    // 1. the tables
    in.mark();
    if (n_out) {
        if ((rc = drv_upload(d, &tb.index, index, n_out))) return rc;
        if ((rc = drv_upload(d, &tb.starts, starts, n_out))) return rc;
        if ((rc = drv_upload(d, &tb.ends, ends, n_out))) return rc;
        if ((rc = drv_upload(d, &tb.xlat, translate, 64))) return rc;
    }
    in.mark();
    // 2. one lane per output; the scan of the lengths.  The packed length is at most n_out times the parent's longest.
    uint64_t key = FZ_REC_NO_ERROR, total = 0, longest = 0;
    in.n = (batch->max_seq_len && n_out > ~0ull / batch->max_seq_len) ? ~0ull : n_out * batch->max_seq_len;
    if (n_out) {
        if ((rc = rec_malloc(&in.starts, n_out))) return rc;
        if ((rc = rec_malloc(&in.at, n_out + 1))) return rc;
        if ((rc = in.arm_verdict())) return rc;
        hipLaunchKernelGGL(fz_derive_measure_kernel, dim3(rec_grid(d, (n_out + FZ_REC_THREADS - 1) / FZ_REC_THREADS)), dim3(FZ_REC_THREADS), 0, d.stream,
                           batch->d_ends_base, n_src, tb.index, tb.starts, tb.ends, n_out, in.starts, in.at, in.info);
        if ((rc = in.scan(in.at, n_out + 1))) return rc;
    }
    in.mark();
    if (n_out && (rc = in.read_verdict(n_out, &key, &total, &longest))) return rc;
    if (key != FZ_REC_NO_ERROR) return drv_report(key, info);
    if (total >= (1ull << FZ_IDX_BITS)) return fail(FZ_EUNSUPPORTED, "sequence too long");
    if (info) { info->packed_bytes = total; info->longest = longest; }
    // 3. the handle, its bytes gathered from the parent's
    const uint8_t *raw = batch->shards[0].d_buf;
    const bool rev = (flags & FZ_DERIVE_REVERSE) != 0;
    fz_seq *seq = nullptr;
    rc = batch_make_handle(ctx, n_out, total, longest, nullptr, in.at, &in.d2h_ms, &seq, [&](uint8_t *d_buf) {
        const dim3 grid(rec_grid(d, (total + FZ_TILE_BYTES - 1) / FZ_TILE_BYTES)), block(FZ_REC_THREADS);
        in.mark();
        if (total) {
            if (tb.xlat && rev)
                hipLaunchKernelGGL((fz_derive_gather_kernel<true, true>), grid, block, 0, d.stream, raw, in.starts, in.at, n_out, total, tb.xlat, d_buf);
            else if (tb.xlat)
                hipLaunchKernelGGL((fz_derive_gather_kernel<false, true>), grid, block, 0, d.stream, raw, in.starts, in.at, n_out, total, tb.xlat, d_buf);
            else if (rev)
                hipLaunchKernelGGL((fz_derive_gather_kernel<true, false>), grid, block, 0, d.stream, raw, in.starts, in.at, n_out, total, tb.xlat, d_buf);
            else                                          // neither: the records gather, the parent's bytes as its text
                hipLaunchKernelGGL(fz_rec_gather_kernel, grid, block, 0, d.stream, raw, in.starts, in.at, n_out, total, d_buf);
        }
        in.mark();
        // a timed call waits for the gather here, so that the host clock around the D2H of ends[] (batch_make_handle) holds
        // the copy and not the gather in front of it on the stream
        if (in.timed) HIP_TRY(hipStreamSynchronize(d.stream));
        return FZ_OK;
    });
    if (rc) return rc;
    if (n_out) { seq->d_src_starts = in.starts; in.starts = nullptr; }
    for (int i = 0; i < 4; ++i) ctx->drv_ms[i] = 0;       // (an untimed call leaves no spans of an earlier one behind)
    if (in.timed) {
        ctx->drv_ms[0] = span_ms(d.rec_ev[0], d.rec_ev[1]);
        ctx->drv_ms[1] = span_ms(d.rec_ev[1], d.rec_ev[2]);
        ctx->drv_ms[2] = span_ms(d.rec_ev[3], d.rec_ev[4]);
        ctx->drv_ms[3] = in.d2h_ms;
    }
    ctx->drv_ms[4] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - in.t_call).count();
    ctx->live.push_back(seq);
    *out = seq;
    return FZ_OK;
}

int fz_debug_derive_ms(fz_ctx *ctx, double *ms5) {
    if (!ctx || !ms5) return fail(FZ_EINVAL, "null argument");
    for (int i = 0; i < 5; ++i) ms5[i] = ctx->drv_ms[i];
    return FZ_OK;
}

int fz_debug_derive_plan(const uint64_t *offs, uint64_t n_src, const uint32_t *index, const uint64_t *starts, const uint64_t *ends,
                         uint64_t n_out, uint64_t *src, uint64_t *at, fz_derive_info *info) {
    if ((!offs && n_src) || ((!src || !at) && n_out) || !info) return fail(FZ_EINVAL, "null argument");
    *info = fz_derive_info{};
    if (int rc = drv_check_args(n_src, index != nullptr, n_out, 0)) return rc;
    info->n_out = n_out;
    uint64_t key = FZ_REC_NO_ERROR, total = 0, longest = 0;
    for (uint64_t j = 0; j < n_out; ++j) {
        const FzDrvItem o = fz_derive_item(offs, n_src, index, starts, ends, j);
        if (o.reason != FZ_REC_OK) key = std::min(key, fz_rec_err_key(j, o.reason));
        src[j] = o.src;
        at[j] = total;
        total += o.len;
        longest = std::max(longest, o.len);
    }
    if (at) at[n_out] = total;
    if (key != FZ_REC_NO_ERROR) return drv_report(key, info);
    if (total >= (1ull << FZ_IDX_BITS)) return fail(FZ_EUNSUPPORTED, "sequence too long");
    info->packed_bytes = total; info->longest = longest;
    return FZ_OK;
}

// ---------------------------------------------------------------------------------------------
// Several lines of every record (fz_batch_upload_records_lines): the text and its line table once (Ingest::line_table),
// then the records path's measure, scan and gather once per kept line.  Every line's measure and scan are enqueued before
// the one readback of all verdicts; with the FASTQ checks the verdict is line 1's, measured even when it is not kept.

namespace {
// One measured line: its tables on the device until a handle takes them.
struct RecPass {
    uint32_t line = 0, flags = 0;
    int out = -1;                                         // the handle it becomes (-1: measured for the verdict only)
    uint64_t n_seqs = 0;                                  // the records it measures
    uint64_t *starts = nullptr, *at = nullptr;
    uint64_t total = 0, longest = 0;
};
struct RecPasses {
    std::vector<RecPass> v;
    ~RecPasses() {
        for (RecPass &p : v)
            for (void *q : {(void *)p.starts, (void *)p.at})
                if (q) (void)hipFree(q);
    }
};

int rec_lines_check_args(const uint8_t *text, uint64_t n, uint32_t period, const uint32_t *lines, uint32_t n_kept, uint32_t flags) {
    if ((!text && n) || !lines) return fail(FZ_EINVAL, "null argument");
    if (flags & ~FZ_REC_FASTQ_CHECKS) return fail(FZ_EINVAL, "unknown record flags");
    if (period == 0 || n_kept == 0 || n_kept > period) return fail(FZ_EINVAL, "between 1 and lines_per_record lines are kept");
    for (uint32_t i = 0; i < n_kept; ++i) {
        if (lines[i] >= period) return fail(FZ_EINVAL, "a kept line must be smaller than lines_per_record");
        for (uint32_t k = 0; k < i; ++k)
            if (lines[k] == lines[i]) return fail(FZ_EINVAL, "line %u is kept twice", lines[i]);
    }
    if ((flags & FZ_REC_FASTQ_CHECKS) && period != 4) return fail(FZ_EINVAL, "the FASTQ checks take 4 lines per record");
    if (n >= (1ull << FZ_IDX_BITS)) return fail(FZ_EUNSUPPORTED, "sequence too long");
    return FZ_OK;
}
}  // namespace

int fz_batch_upload_records_lines(fz_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t lines_per_record, const uint32_t *lines,
                                  uint32_t n_kept, uint32_t flags, fz_seq **outs, fz_records_info *info) {
    if (!ctx || !outs) return fail(FZ_EINVAL, "null argument");
    if (info) *info = fz_records_info{};
    int rc = rec_lines_check_args(text, n, lines_per_record, lines, n_kept, flags);
    if (rc) return rc;                                    // (n_kept is not known to be the length of outs[] before this)
    for (uint32_t i = 0; i < n_kept; ++i) outs[i] = nullptr;
    if ((rc = batch_upload_admit(ctx))) return rc;
    Ingest in(ctx, "records");
    DevState &d = in.d;
    const bool checks = (flags & FZ_REC_FASTQ_CHECKS) != 0;
    if (checks) n = rec_trim(text, n);
    // 1. the line table, once
    uint64_t n_nl = 0, n_lines = 0;
    if ((rc = in.line_table(text, n, &n_nl, &n_lines))) return rc;
    uint64_t n_seqs = ~0ull;                              // the records in which every kept line exists
    for (uint32_t i = 0; i < n_kept; ++i) n_seqs = std::min(n_seqs, fz_rec_n_seqs(n_lines, lines_per_record, lines[i]));
    if (info) { info->n_lines = n_lines; info->n_seqs = n_seqs; }
    if (n_seqs >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "more than 2^32 - 1 sequences in a batch");
    // 2. one lane per record and the scan of the lengths, per line; line 1 carries the FASTQ verdict
    RecPasses ps;
    bool has_verdict_line = false;
    for (uint32_t i = 0; i < n_kept; ++i) has_verdict_line |= lines[i] == 1u;
    if (checks && !has_verdict_line) {                    // (over the records whose line 1 exists, as the single-line call)
        ps.v.emplace_back();
        ps.v.back().line = 1u; ps.v.back().flags = flags; ps.v.back().n_seqs = fz_rec_n_seqs(n_lines, lines_per_record, 1u);
    }
    for (uint32_t i = 0; i < n_kept; ++i) {
        ps.v.emplace_back();
        ps.v.back().line = lines[i]; ps.v.back().out = (int)i; ps.v.back().n_seqs = n_seqs;
        ps.v.back().flags = (checks && lines[i] == 1u) ? flags : 0u;
    }
    const size_t np = ps.v.size();
    uint64_t key = fz_rec_count_key(n_lines, lines_per_record, flags);
    bool measured = false;
    if ((rc = rec_malloc(&in.info, 2 * np))) return rc;
    for (size_t i = 0; i < np; ++i) {
        RecPass &p = ps.v[i];
        if (!p.n_seqs) continue;
        measured = true;
        if ((rc = rec_malloc(&p.starts, p.n_seqs))) return rc;
        if ((rc = rec_malloc(&p.at, p.n_seqs + 1))) return rc;
        HIP_TRY(hipMemsetAsync(in.info + 2 * i, 0xff, sizeof(uint64_t), d.stream));
        HIP_TRY(hipMemsetAsync(in.info + 2 * i + 1, 0, sizeof(uint64_t), d.stream));
        hipLaunchKernelGGL(fz_rec_measure_kernel, dim3(rec_grid(d, (p.n_seqs + FZ_REC_THREADS - 1) / FZ_REC_THREADS)), dim3(FZ_REC_THREADS), 0, d.stream,
                           in.raw, n, in.nl, n_nl, n_lines, lines_per_record, p.line, p.flags, p.n_seqs, p.starts, p.at, in.info + 2 * i);
        if ((rc = in.scan(p.at, p.n_seqs + 1))) return rc;
    }
    in.mark();
    if (measured) {
        std::vector<unsigned long long> got(2 * np, 0ull);
        HIP_TRY(hipMemcpyAsync(got.data(), in.info, got.size() * sizeof(got[0]), hipMemcpyDeviceToHost, d.stream));
        for (RecPass &p : ps.v)
            if (p.n_seqs) HIP_TRY(hipMemcpyAsync(&p.total, p.at + p.n_seqs, sizeof(uint64_t), hipMemcpyDeviceToHost, d.stream));
        HIP_TRY(hipStreamSynchronize(d.stream));
        for (size_t i = 0; i < np; ++i) {
            if (!ps.v[i].n_seqs) continue;
            key = std::min<uint64_t>(key, got[2 * i]);
            ps.v[i].longest = got[2 * i + 1];
        }
        if (key == FZ_REC_NO_ERROR)
            for (const RecPass &p : ps.v)
                if (p.total > n || p.longest > p.total) return fail(FZ_EDEVICE, "records: the packed length is outside the text");
    }
    if (key != FZ_REC_NO_ERROR) return rec_report(checks ? "fastq" : "lines", key, info);
    // 3. the handles, their bytes gathered on the device
    double kernels_ms = 0, d2h_ms = 0;
    std::vector<fz_seq *> made;
    for (RecPass &p : ps.v) {
        if (p.out < 0) continue;
        fz_seq *seq = nullptr;
        double one_d2h = 0;
        const uint64_t *at = p.at;                        // (batch_make_handle takes p.at over: the gather is enqueued before that)
        rc = batch_make_handle(ctx, n_seqs, p.total, p.longest, nullptr, p.at, &one_d2h, &seq, [&](uint8_t *d_buf) {
            if (in.timed) (void)hipEventRecord(d.rec_ev[5], d.stream);
            if (p.total)
                hipLaunchKernelGGL(fz_rec_gather_kernel, dim3(rec_grid(d, (p.total + FZ_TILE_BYTES - 1) / FZ_TILE_BYTES)), dim3(FZ_REC_THREADS), 0,
                                   d.stream, in.raw, p.starts, at, n_seqs, p.total, d_buf);
            if (in.timed) (void)hipEventRecord(d.rec_ev[6], d.stream);
            return FZ_OK;
        });
        if (rc) break;
        if (n_seqs) { seq->d_src_starts = p.starts; p.starts = nullptr; }
        if (in.timed) kernels_ms += span_ms(d.rec_ev[5], d.rec_ev[6]);      // (the handle's builder has waited for the stream)
        d2h_ms += one_d2h;
        made.push_back(seq);
        if (p.out == 0 && info) info->packed_bytes = p.total;
    }
    if (rc) {
        for (fz_seq *s : made) fz_seq_release(s);
        if (info) info->packed_bytes = 0;
        return rc;
    }
    if (in.timed) {
        ctx->rec_ms[0] = span_ms(d.rec_ev[0], d.rec_ev[1]);
        ctx->rec_ms[1] = span_ms(d.rec_ev[1], d.rec_ev[2]) + span_ms(d.rec_ev[3], d.rec_ev[4]) + kernels_ms;
        ctx->rec_ms[2] = d2h_ms;
    }
    ctx->rec_ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - in.t_call).count();
    size_t k = 0;
    for (const RecPass &p : ps.v)
        if (p.out >= 0) { ctx->live.push_back(made[k]); outs[p.out] = made[k]; ++k; }
    return FZ_OK;
}

// ---------------------------------------------------------------------------------------------
// Formatted text (fz_batch_format): the egress end.  The descriptor goes up, one lane per record measures and checks it
// (fz_kernels.h: fz_format_measure_kernel), the records path's scan places the records, the gather writes the text into a
// transient buffer of whole tiles, and one copy brings it to the caller's buffer.

namespace {
static_assert(sizeof(fz_format_info) == 40, "fz_format_info");
static_assert(FZ_FMT_MAX_COLS == FZ_FORMAT_MAX_COLUMNS && FZ_FMT_MAX_LIT == FZ_FORMAT_MAX_LITERAL && FZ_FMT_NO_CHECK == FZ_FORMAT_NO_CHECK,
              "fz_device.h and fzhip.h state the same limits");

const char *fmt_reason_text(uint32_t reason) {
    if (reason == FZ_FMT_E_EQUAL) return "the two columns checked for equal length differ in length";
    return "bad record";
}

int fmt_report(uint64_t key, fz_format_info *info) {
    if (info) { info->bad_record = fz_rec_err_record(key); info->bad_reason = fz_rec_err_reason(key); }
    return fail(FZ_EINVAL, "format: record %llu: %s", (unsigned long long)fz_rec_err_record(key), fmt_reason_text(fz_rec_err_reason(key)));
}

// The descriptor's host half: the literals and the pair to check.  -> the literals' total per record.
int fmt_describe(uint32_t n_columns, const uint8_t *literals, const uint32_t *literal_lens, uint32_t equal_a, uint32_t equal_b,
                 FzFmtDesc &desc, uint64_t *lit_total) {
    if (n_columns == 0 || n_columns > FZ_FMT_MAX_COLS) return fail(FZ_EINVAL, "between 1 and %u columns are formatted", FZ_FMT_MAX_COLS);
    if (!literal_lens) return fail(FZ_EINVAL, "null argument");
    memset(&desc, 0, sizeof desc);
    desc.n_cols = n_columns;
    uint32_t at = 0;
    for (uint32_t c = 0; c <= n_columns; ++c) {
        if (literal_lens[c] > FZ_FMT_MAX_LIT) return fail(FZ_EINVAL, "literal %u is longer than %u bytes", c, FZ_FMT_MAX_LIT);
        desc.lit_off[c] = at;
        at += literal_lens[c];
    }
    desc.lit_off[n_columns + 1u] = at;
    if (at && !literals) return fail(FZ_EINVAL, "null argument");
    if (at && literals) memcpy(desc.lits, literals, at);
    const bool check = equal_a != FZ_FMT_NO_CHECK && equal_b != FZ_FMT_NO_CHECK;
    if (check && (equal_a >= n_columns || equal_b >= n_columns)) return fail(FZ_EINVAL, "the columns checked for equal length are columns of the call");
    desc.equal_a = check ? equal_a : FZ_FMT_NO_CHECK;
    desc.equal_b = check ? equal_b : FZ_FMT_NO_CHECK;
    *lit_total = at;
    return FZ_OK;
}

// sum + n * lit_total, or ~0 when it does not fit.
uint64_t fmt_text_bytes(uint64_t sum, uint64_t n, uint64_t lit_total) {
    if (lit_total && n > (~0ull - sum) / lit_total) return ~0ull;
    return sum + n * lit_total;
}

struct FmtTables {
    FzFmtDesc *desc = nullptr;
    ~FmtTables() { if (desc) (void)hipFree(desc); }
};
}  // namespace

int fz_batch_format(fz_ctx *ctx, fz_seq *const *columns, uint32_t n_columns, const uint8_t *literals, const uint32_t *literal_lens,
                    uint32_t equal_a, uint32_t equal_b, uint8_t *out, uint64_t cap, fz_format_info *info) {
    if (!ctx || !columns) return fail(FZ_EINVAL, "null argument");
    if (info) *info = fz_format_info{};
    int rc = batch_upload_admit(ctx);
    if (rc) return rc;
    FzFmtDesc desc;
    uint64_t lit_total = 0, sum = 0;
    if ((rc = fmt_describe(n_columns, literals, literal_lens, equal_a, equal_b, desc, &lit_total))) return rc;
    for (uint32_t c = 0; c < n_columns; ++c) {
        fz_seq *col = columns[c];
        if (!col || std::find(ctx->live.begin(), ctx->live.end(), col) == ctx->live.end())
            return fail(FZ_EINVAL, "fz_batch_format: column %u is no live batch handle of this context", c);
        if (!col->is_batch) return fail(FZ_EINVAL, "fz_batch_format: column %u is no batch handle", c);
        if (col->shards.size() != 1) return fail(FZ_EUNSUPPORTED, "batches are formatted on one device");
        if (col->n_seqs != columns[0]->n_seqs)
            return fail(FZ_EINVAL, "fz_batch_format: column %u has %llu sequences, column 0 has %llu", c, (unsigned long long)col->n_seqs,
                        (unsigned long long)columns[0]->n_seqs);
        sum += col->n;                                    // (each below 2^48, at most 8 of them)
        desc.col[c].bytes = col->shards[0].d_buf;
        desc.col[c].offs = col->d_ends_base;
    }
    const uint64_t n = columns[0]->n_seqs;
    const uint64_t text_bytes = fmt_text_bytes(sum, n, lit_total);
    if (text_bytes >= (1ull << FZ_IDX_BITS)) return fail(FZ_EUNSUPPORTED, "the text is too long");
    if (info) { info->n_records = n; info->text_bytes = text_bytes; }
    if (cap < text_bytes) return fail(FZ_EINVAL, "the buffer is smaller than the text");
    if (!out && text_bytes) return fail(FZ_EINVAL, "null argument");
    Ingest in(ctx, "format");
    DevState &d = in.d;
    FmtTables tb;
    HIP_TRY(hipSetDevice(d.device));
    if (in.timed) for (auto &ev : d.rec_ev) if (!ev) HIP_TRY(hipEventCreate(&ev));
    // 1. the descriptor
    in.mark();
    if (n) {
        if ((rc = rec_malloc_bytes(reinterpret_cast<void **>(&tb.desc), sizeof desc))) return rc;
        HIP_TRY(hipMemcpyAsync(tb.desc, &desc, sizeof desc, hipMemcpyHostToDevice, d.stream));
    }
    in.mark();
    // 2. one lane per record; the scan of the lengths
    uint64_t key = FZ_REC_NO_ERROR, total = 0, longest = 0;
    in.n = text_bytes;
    if (n) {
        if ((rc = rec_malloc(&in.at, n + 1))) return rc;
        if ((rc = in.arm_verdict())) return rc;
        hipLaunchKernelGGL(fz_format_measure_kernel, dim3(rec_grid(d, (n + FZ_REC_THREADS - 1) / FZ_REC_THREADS)), dim3(FZ_REC_THREADS), 0, d.stream,
                           tb.desc, n, in.at, in.info);
        if ((rc = in.scan(in.at, n + 1))) return rc;
    }
    in.mark();
    if (n && (rc = in.read_verdict(n, &key, &total, &longest))) return rc;
    if (key != FZ_REC_NO_ERROR) return fmt_report(key, info);
    if (total != text_bytes) return fail(FZ_EDEVICE, "format: the measured length is not the text's");
    if (info) info->longest_record = longest;
    // 3. the text, gathered into whole tiles, and its copy to the caller
    double d2h_ms = 0;
    in.mark();
    if (total) {
        const uint64_t ntiles = (total + FZ_TILE_BYTES - 1) / FZ_TILE_BYTES;
        if ((rc = rec_malloc_bytes(reinterpret_cast<void **>(&in.raw), ntiles * FZ_TILE_BYTES))) return rc;
        hipLaunchKernelGGL(fz_format_gather_kernel, dim3(rec_grid(d, ntiles)), dim3(FZ_REC_THREADS), 0, d.stream, tb.desc, in.at, n, total, in.raw);
    }
    in.mark();
    if (total) {
        // a timed call waits for the gather here, so that the host clock around the copy holds the copy alone
        if (in.timed) HIP_TRY(hipStreamSynchronize(d.stream));
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipMemcpyAsync(out, in.raw, total, hipMemcpyDeviceToHost, d.stream));
        HIP_TRY(hipStreamSynchronize(d.stream));
        d2h_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    for (int i = 0; i < 4; ++i) ctx->fmt_ms[i] = 0;       // (an untimed call leaves no spans of an earlier one behind)
    if (in.timed) {
        ctx->fmt_ms[0] = span_ms(d.rec_ev[0], d.rec_ev[1]);
        ctx->fmt_ms[1] = span_ms(d.rec_ev[1], d.rec_ev[2]);
        ctx->fmt_ms[2] = span_ms(d.rec_ev[3], d.rec_ev[4]);
        ctx->fmt_ms[3] = d2h_ms;
    }
    ctx->fmt_ms[4] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - in.t_call).count();
    return FZ_OK;
}

int fz_debug_format_ms(fz_ctx *ctx, double *ms5) {
    if (!ctx || !ms5) return fail(FZ_EINVAL, "null argument");
    for (int i = 0; i < 5; ++i) ms5[i] = ctx->fmt_ms[i];
    return FZ_OK;
}

int fz_debug_format_plan(const uint64_t *const *offs, uint32_t n_columns, uint64_t n, const uint32_t *literal_lens,
                         uint32_t equal_a, uint32_t equal_b, uint64_t *at, fz_format_info *info) {
    if (!offs || !at || !info) return fail(FZ_EINVAL, "null argument");
    *info = fz_format_info{};
    FzFmtDesc desc;
    uint64_t lit_total = 0, sum = 0;
    static const uint8_t no_bytes[(FZ_FMT_MAX_COLS + 1u) * FZ_FMT_MAX_LIT] = {};
    if (int rc = fmt_describe(n_columns, no_bytes, literal_lens, equal_a, equal_b, desc, &lit_total)) return rc;
    for (uint32_t c = 0; c < n_columns; ++c) {
        if (!offs[c]) return fail(FZ_EINVAL, "null argument");
        desc.col[c].offs = offs[c];
        sum += offs[c][n] - offs[c][0];
    }
    const uint64_t text_bytes = fmt_text_bytes(sum, n, lit_total);
    if (text_bytes >= (1ull << FZ_IDX_BITS)) return fail(FZ_EUNSUPPORTED, "the text is too long");
    info->n_records = n; info->text_bytes = text_bytes;
    uint64_t key = FZ_REC_NO_ERROR, total = 0, longest = 0;
    for (uint64_t j = 0; j < n; ++j) {
        const FzFmtRec o = fz_format_record(desc, j);
        if (o.reason != FZ_REC_OK) key = std::min(key, fz_rec_err_key(j, o.reason));
        at[j] = total;
        total += o.len;
        longest = std::max(longest, o.len);
    }
    at[n] = total;
    if (key != FZ_REC_NO_ERROR) return fmt_report(key, info);
    info->longest_record = longest;
    return FZ_OK;
}

int fz_search_exact(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint64_t lo, uint64_t hi,
                    uint64_t **idx, uint64_t *n) {
    if (!idx || !n) return fail(FZ_EINVAL, "null argument");
    *idx = nullptr; *n = 0;
    int rc = validate(ctx, seq, p, m);
    if (rc) return rc;
    rc = check_halo(seq, m);
    if (rc) return rc;
    const uint64_t N = seq->n;
    lo = std::min(lo, N);                                  // search_exact.py:70-71
    hi = std::max(lo, std::min(hi, N));
    Search q;
    q.mode = FZ_MODE_EXACT; q.m = m; q.k = 0; q.p = p;
    q.plan.L = m;
    q.plan.s = {0};
    q.plan.abs_lo = lo;
    q.plan.abs_hi = hi;
    std::vector<FzRec> recs;
    std::vector<uint64_t> hits;
    rc = run_search(ctx, seq, q, /*with_verify=*/false, recs, hits);
    if (rc) return rc;
    if (comm_multi_process(ctx)) {                         // one rank of several: every rank gets every rank's hits
        std::vector<uint8_t> all;
        rc = comm_gather_host(ctx, hits.data(), hits.size() * sizeof(uint64_t), all);
        if (rc) return rc;
        hits.resize(all.size() / sizeof(uint64_t));
        if (!all.empty()) memcpy(hits.data(), all.data(), all.size());
    }
    std::sort(hits.begin(), hits.end());
    void *mem = nullptr;
    rc = alloc_out(hits.size(), sizeof(uint64_t), &mem);
    if (rc) return rc;
    uint64_t *o = static_cast<uint64_t *>(mem);
    for (size_t i = 0; i < hits.size(); ++i) o[i] = fz_hit_index(hits[i]);
    *idx = o; *n = hits.size();
    ctx->stats.raw_matches = hits.size();
    return FZ_OK;
}

// Argument checks and the block plan of find_near_matches_levenshtein_ngrams (levenshtein_ngram.py:159-176).
static int lev_plan(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, Search &q, bool in_pipeline = false) {
    int rc = validate(ctx, seq, p, m, in_pipeline);
    if (rc) return rc;
    const uint32_t L = m / (k + 1);
    if (L == 0) return fail(FZ_EINVAL, "the subsequence length must be greater than max_l_dist");
    if (k > FZ_MAX_K_ANY) return fail(FZ_EUNSUPPORTED, "max_l_dist above %u is not supported by the verify kernels", FZ_MAX_K_ANY);
    rc = check_halo(seq, (uint64_t)m + k);
    if (rc) return rc;
    q.mode = FZ_MODE_LEV; q.m = m; q.k = k; q.p = p;
    q.collective = ctx->snapshot;
    q.plan.L = L;
    for (uint32_t s = 0; s + L <= m; s += L) q.plan.s.push_back(s);   // levenshtein_ngram.py:171-176 (ranges: fz_block_range)
    if (q.plan.s.size() > FZ_MAX_BLOCKS) return fail(FZ_EUNSUPPORTED, "more than %u n-gram blocks", FZ_MAX_BLOCKS);
    return FZ_OK;
}

// Argument checks and the block plan of the substitutions-only n-gram search (template :92-101).
static int subs_plan(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, Search &q, bool in_pipeline = false) {
    int rc = validate(ctx, seq, p, m, in_pipeline);
    if (rc) return rc;
    const uint32_t L = m / (k + 1);
    if (L == 0) return fail(FZ_EUNSUPPORTED, "max_substitutions >= len(subsequence): every window matches; not a GPU path");
    rc = check_halo(seq, m);
    if (rc) return rc;
    q.mode = FZ_MODE_SUBS; q.m = m; q.k = k; q.p = p;
    q.collective = ctx->snapshot;
    q.plan.L = L;
    for (uint32_t s = 0; s + L <= m; s += L) q.plan.s.push_back(s);   // template :92-101 (ranges: fz_block_range)
    if (q.plan.s.size() > FZ_MAX_BLOCKS) return fail(FZ_EUNSUPPORTED, "more than %u n-gram blocks", FZ_MAX_BLOCKS);
    return FZ_OK;
}

int fz_lev_ngrams(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, fz_match **out, uint64_t *n) {
    if (!out || !n) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *n = 0;
    Search q;
    int rc = lev_plan(ctx, seq, p, m, k, q);
    if (rc) return rc;
    std::vector<FzRec> recs;
    std::vector<uint64_t> hits;
    Trace tr;
    rc = run_search(ctx, seq, q, true, recs, hits);
    if (rc) return rc;
    tr.mark("run_search");
    rc = emit_matches(ctx, recs, q.plan.L, out, n, seq->n, (uint32_t)q.plan.s.size());
    tr.mark("sort+emit");
    if (rc == FZ_OK) ctx->stats.raw_matches = *n;
    return rc;
}

// find_near_matches_levenshtein_ngrams + consolidate_overlapping_matches in one call (what LevenshteinSearch.search followed
// by consolidate_matches computes): no second call, no array round trip through the caller in between.
int fz_lev_ngrams_consolidated(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, fz_match **out, uint64_t *n) {
    if (!out || !n) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *n = 0;
    fz_match *raw = nullptr;
    uint64_t nraw = 0;
    int rc = fz_lev_ngrams(ctx, seq, p, m, k, &raw, &nraw);
    if (rc) return rc;
    rc = fz_consolidate(raw, nraw, out, n);
    release_out(raw);
    return rc;
}

// ---------------------------------------------------------------------------------------------
// Multi-pattern search: many patterns, one budget, one resident sequence, as few passes over it as the patterns allow
// (fz_device.h: the fz_mp_* table; fz_kernels.h: fz_mp_filter_kernel / fz_mp_verify_kernel / fz_mp_verify_subs_kernel).
// The filter knows nothing about the distance; `mode` (FZ_MODE_LEV or FZ_MODE_SUBS) picks the verification kernel, the
// window a candidate needs and the cost rule's constants.

// Where every pattern of a list rides: a function of the arguments alone.  Patterns inside the batched domain are grouped by
// their n-gram length L = m / (k + 1) in input order; a group is closed when the next pattern of its L would take it beyond
// FZ_MP_MAX_PATS patterns or FZ_MP_MAX_BLOCKS blocks.  A group of one pattern, and every pattern outside the domain, takes
// the single-pattern route, and so does a group that the cost rule below gives to the loop.  Groups are numbered in the order
// of their first pattern.
struct MpGroup { uint32_t L = 0, blocks = 0; std::vector<uint32_t> pats; };

// (The same domain for both modes.  Hamming verification has no register band and would take k above FZ_MP_MAX_K; nothing
// measured asks for it yet, so substitutions keep the Levenshtein domain.)
static bool mp_in_domain(uint32_t mode, uint32_t m, uint32_t k) {
    (void)mode;
    return k >= 1 && k <= FZ_MP_MAX_K && m <= FZ_MP_MAX_M && m / (k + 1) >= FZ_MP_MIN_L;
}

// Is one pass for the group expected to beat one search per pattern?  Both sides in ms per GiB, from the measurement of
// profiles/r08_multi_pattern.txt (1 GiB of DNA), as functions of the arguments: P patterns, G blocks and
// the project's estimate of expected candidates, C = G / sigma^L of the offsets (sigma = distinct symbols of the group's
// patterns), in millions per GiB:
//     one pass      kMpPass + kMpPerBlock G + kMpPerCand C     (the filter's rare path grows with the blocks, the hit list
//                                                                and the lane-per-candidate verification with the candidates)
//     the loop      kLoopScan P + kLoopPerCand C               (a scan per pattern; its fused verification per candidate)
// The group rides one pass when that is expected to cost less than kMpMargin of the loop.
constexpr double kMpPass = 0.50, kMpPerBlock = 0.0098, kMpPerCand = 0.085;
constexpr double kLoopScan = 0.185, kLoopPerCand = 0.032;
constexpr double kMpMargin = 0.9;
// Substitutions only (profiles/r10_multi_pattern_subs.txt, the same 1 GiB of DNA, every cell forced onto a pass; DESIGN.md
// section 6).  The pass keeps the filter's terms — it is the same kernel.  The loop is one synchronous fz_subs_ngrams per
// pattern: 0.201 P + 0.031 C by least squares over the sixteen cells (residuals below 9 %).  The pass's cost per candidate
// is not a constant — 0.062 ms per million at 3 M candidates, 0.016 at 268 M: the filter's rare path saturates — so it is
// set where the rule decides: every value in [0.032, 0.054] sends each of the sixteen cells where it measured faster, and
// the constant is the middle of that interval.
constexpr double kMpSubsPerCand = 0.043;
constexpr double kLoopSubsScan = 0.201, kLoopSubsPerCand = 0.031;

// The distinct symbols of a group's patterns.
static uint32_t mp_sigma(const uint8_t *pats, const uint64_t *offs, const MpGroup &g) {
    bool seen[256] = {false};
    uint32_t sigma = 0;
    for (uint32_t i : g.pats)
        for (uint64_t q = offs[i]; q < offs[i + 1]; ++q)
            if (!seen[pats[q]]) { seen[pats[q]] = true; ++sigma; }
    return sigma;
}

static bool mp_worth_a_pass(uint32_t mode, const uint8_t *pats, const uint64_t *offs, const MpGroup &g) {
    const uint32_t sigma = mp_sigma(pats, offs, g);
    double frac = (double)g.blocks;
    for (uint32_t i = 0; i < g.L && frac > 1e-12; ++i) frac /= (double)sigma;
    const double cand = std::min(frac, (double)g.blocks) * 1073.741824;      // millions per GiB
    const bool subs = mode == FZ_MODE_SUBS;
    const double pass = kMpPass + kMpPerBlock * g.blocks + (subs ? kMpSubsPerCand : kMpPerCand) * cand;
    const double loop = (subs ? kLoopSubsScan : kLoopScan) * (double)g.pats.size() + (subs ? kLoopSubsPerCand : kLoopPerCand) * cand;
    return pass < kMpMargin * loop;
}

static void mp_plan(uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k, std::vector<MpGroup> &groups,
                    std::vector<uint32_t> &group_of) {
    groups.clear();
    group_of.assign(n_pats, 0xffffffffu);
    std::vector<MpGroup> open;                                  // at most one open group per L
    std::vector<MpGroup> closed;
    auto close = [&](MpGroup &g) { if (g.pats.size() > 1 && (sw().mp_force_pass || mp_worth_a_pass(mode, pats, offs, g))) closed.push_back(g); };
    for (uint32_t i = 0; i < n_pats; ++i) {
        const uint64_t m64 = offs[i + 1] - offs[i];
        if (m64 > FZ_MP_MAX_M || !mp_in_domain(mode, (uint32_t)m64, k)) continue;
        const uint32_t m = (uint32_t)m64, L = m / (k + 1), nb = m / L;
        MpGroup *g = nullptr;
        for (MpGroup &o : open) if (o.L == L) g = &o;
        if (g && (g->pats.size() + 1 > FZ_MP_MAX_PATS || g->blocks + nb > FZ_MP_MAX_BLOCKS)) {
            close(*g);
            g->pats.clear();
            g->blocks = 0;
        }
        if (!g) { open.emplace_back(); g = &open.back(); g->L = L; }
        g->pats.push_back(i);
        g->blocks += nb;
    }
    for (MpGroup &o : open) close(o);
    std::sort(closed.begin(), closed.end(), [](const MpGroup &x, const MpGroup &y) { return x.pats[0] < y.pats[0]; });
    groups.swap(closed);
    for (uint32_t gi = 0; gi < groups.size(); ++gi)
        for (uint32_t i : groups[gi].pats) group_of[i] = gi;
}

// Symbol classes of a call (fz_*_cls; fz_device.h: the class descriptor): the caller's two 256-byte tables.
struct MpCls { const uint8_t *pmask, *tmask; };

static int mp_check_cls(const uint8_t *pmask, const uint8_t *tmask) {
    if (!pmask || !tmask) return fail(FZ_EINVAL, "null argument");
    uint32_t seen = 0;
    for (uint32_t t = 0; t < 256; ++t) {
        if (tmask[t] & (tmask[t] - 1u)) return fail(FZ_EINVAL, "tmask[%u] has more than one bit", t);
        if (tmask[t] & seen) return fail(FZ_EINVAL, "tmask[%u] repeats the bit of another base symbol", t);
        seen |= tmask[t];
    }
    return FZ_OK;
}

// mp_plan for a call with classes.  Every pattern rides a pass — the single-pattern route knows no classes, so the cost
// rule is not consulted and a group of one is a group — and so every pattern has to be inside the batched domain.  A group's
// `blocks` are its table entries, expansions included (fz_mp_cls_entries): it is closed when the next pattern of its L would
// take it beyond FZ_MP_MAX_PATS patterns or FZ_MP_MAX_BLOCKS entries.  pat_entries (optional): the entries of every pattern.
static int mp_plan_cls(const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k, const MpCls &cls, std::vector<MpGroup> &groups,
                       std::vector<uint32_t> &group_of, uint32_t *pat_entries = nullptr) {
    groups.clear();
    group_of.assign(n_pats, 0xffffffffu);
    std::vector<MpGroup> open, closed;
    for (uint32_t i = 0; i < n_pats; ++i) {
        const uint64_t m64 = offs[i + 1] - offs[i];
        if (m64 > FZ_MP_MAX_M || !mp_in_domain(FZ_MODE_SUBS, (uint32_t)m64, k))
            return fail(FZ_EUNSUPPORTED, "pattern %u (length %llu, %u substitutions) is outside the multi-pattern domain "
                        "1 <= k <= %u, m <= %u, m / (k + 1) >= %u: symbol classes are searched there only", i, (unsigned long long)m64, k,
                        FZ_MP_MAX_K, FZ_MP_MAX_M, FZ_MP_MIN_L);
        const uint32_t m = (uint32_t)m64, L = m / (k + 1);
        const uint32_t ne = fz_mp_cls_entries(pats + offs[i], m, L, cls.pmask, cls.tmask);
        if (ne > FZ_MP_MAX_BLOCKS)
            return fail(FZ_EUNSUPPORTED, "pattern %u: the spellings of its n-gram blocks need more than %u table entries "
                        "(too many class symbols within the first 8 bytes of a block)", i, FZ_MP_MAX_BLOCKS);
        if (pat_entries) pat_entries[i] = ne;
        MpGroup *g = nullptr;
        for (MpGroup &o : open) if (o.L == L) g = &o;
        if (g && (g->pats.size() + 1 > FZ_MP_MAX_PATS || g->blocks + ne > FZ_MP_MAX_BLOCKS)) {
            closed.push_back(*g);
            g->pats.clear();
            g->blocks = 0;
        }
        if (!g) { open.emplace_back(); g = &open.back(); g->L = L; }
        g->pats.push_back(i);
        g->blocks += ne;
    }
    for (MpGroup &o : open) if (!o.pats.empty()) closed.push_back(o);
    std::sort(closed.begin(), closed.end(), [](const MpGroup &x, const MpGroup &y) { return x.pats[0] < y.pats[0]; });
    groups.swap(closed);
    for (uint32_t gi = 0; gi < groups.size(); ++gi)
        for (uint32_t i : groups[gi].pats) group_of[i] = gi;
    return FZ_OK;
}

static int mp_ensure(DevState &d, uint64_t hit_cap, uint64_t rec_cap, uint32_t desc_words = FZ_MP_DESC_WORDS) {
    HIP_TRY(hipSetDevice(d.device));
    if (d.d_mp_desc && d.mp_desc_words < desc_words) {         // (the stream is idle between group launches)
        HIP_TRY(hipFree(d.d_mp_desc));
        d.d_mp_desc = nullptr;
        d.mp_desc_words = 0;
    }
    if (!d.d_mp_desc) {
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d.d_mp_desc), (size_t)desc_words * 4u));
        d.mp_desc_words = desc_words;
    }
    if (!d.d_mp_ctr) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d.d_mp_ctr), FZ_MP_CTR_WORDS * 8u));
    int rc = grow_device(d, d.d_mp_hits, d.mp_hit_cap, hit_cap, (uint64_t)FZ_MP_LISTS * hit_cap * sizeof(uint64_t));
    if (rc) return rc;
    return grow_device(d, d.d_mp_recs, d.mp_rec_cap, rec_cap, rec_cap * sizeof(FzRec));
}

// What a list-of-patterns call reports (fz_stats): summed over its group launches and its single searches.
struct MpTotals {
    uint64_t bytes = 0, hits = 0, rows = 0;
    uint32_t launches = 0;
    double filter_ms = 0, verify_ms = 0;
    // a finished single search, from the stats it left (its rows are the caller's to count; its spans are not summed)
    void add_search(const fz_stats_t &st) { bytes += st.bytes_scanned; hits += st.ngram_hits; launches += st.filter_launches; }
};

// The totals become the context's stats.  raw_matches: the rows (or, for an assignment, the records folded);
// extra_verify_ms: kernels behind the verification that count with it (the assignment's fold).
static void mp_publish(fz_ctx *ctx, const MpTotals &tot, uint64_t raw_matches, uint32_t form, double extra_verify_ms = 0) {
    memset(&ctx->stats, 0, sizeof ctx->stats);
    ctx->tref.clear();
    ctx->stats.n_devices = (uint32_t)ctx->devs.size();
    ctx->stats.filter_launches = tot.launches;
    ctx->stats.bytes_scanned = tot.bytes;
    ctx->stats.ngram_hits = tot.hits;
    ctx->stats.raw_matches = raw_matches;
    ctx->stats.filter_ms = tot.filter_ms;
    ctx->stats.verify_ms = tot.verify_ms + extra_verify_ms;
    ctx->stats.device_ms = tot.filter_ms + tot.verify_ms + extra_verify_ms;
    ctx->stats.verify_form = form;
}

// One group over one shard: descriptor up, filter, verification, counters and records back.  Capacities come from the
// arguments — the project's estimate of expected candidates, sequence bytes x blocks / sigma^L (sigma = distinct symbols
// of the group's patterns), twice over and spread over the lists; a launch that overflows a list or the record buffer is
// run again with what its counters ask for.
// -> *n_recs records in d.d_mp_recs (the attempt that did not overflow), the stream idle.
static int mp_launch_shard(fz_ctx *ctx, const Shard &sh, uint32_t mode, const uint32_t *desc, uint32_t nent, uint32_t k, uint32_t L, uint32_t max_m,
                           uint32_t sigma, uint64_t *n_recs, MpTotals &tot, bool rag = false, bool cls = false) {
    DevState &d = ctx->devs[sh.dev];
    *n_recs = 0;
    const uint64_t ntiles = (sh.geom.buf_len + FZ_TILE_BYTES - 1) / FZ_TILE_BYTES;
    tot.bytes += sh.geom.buf_len;
    if (ntiles == 0) return FZ_OK;
    double expect = (double)sh.geom.buf_len * (double)nent;
    for (uint32_t i = 0; i < L && expect > 1.0; ++i) expect /= (double)sigma;
    uint64_t hit_cap = std::max<uint64_t>(4096, (uint64_t)(2.0 * expect / FZ_MP_LISTS) + 1024);
    uint64_t rec_cap = 1u << 16;
    FzMpArgs a;
    memset(&a, 0, sizeof a);
    a.geom = sh.geom;
    a.k = k; a.L = L; a.nent = nent;
    const bool subs = mode == FZ_MODE_SUBS;
    a.win_dwords = subs ? (max_m + 3) / 4 + 1 : (max_m + 2 * k + 6) / 4 + 1;
    using FilterKernel = void (*)(const uint8_t *, const FzMpArgs, uint64_t, const uint32_t *, uint64_t *, unsigned long long *);
    static const FilterKernel filters[6] = {nullptr, fz_mp_filter_kernel<1>, fz_mp_filter_kernel<2>, fz_mp_filter_kernel<3>,
                                            fz_mp_filter_kernel<4>, fz_mp_filter_kernel<5>};
    const FilterKernel fk = filters[fz_mp_dh(L)];
    // (cls: desc is a class descriptor — the filter reads its first part as ever, the class kernels the whole of it)
    const uint32_t desc_words = cls ? FZ_MP_CLS_DESC_WORDS : FZ_MP_DESC_WORDS;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(ntiles, (uint64_t)d.n_cus * 8);
    for (int attempt = 0; attempt < 4; ++attempt) {
        int rc = mp_ensure(d, hit_cap, rec_cap, desc_words);
        if (rc) return rc;
        a.hit_cap = d.mp_hit_cap;
        a.rec_cap = d.mp_rec_cap;
        const uint32_t *ddesc = reinterpret_cast<const uint32_t *>(d.d_mp_desc);
        unsigned long long *dctr = reinterpret_cast<unsigned long long *>(d.d_mp_ctr);
        HIP_TRY(hipMemcpyAsync(d.d_mp_desc, desc, (size_t)desc_words * 4u, hipMemcpyHostToDevice, d.stream));
        HIP_TRY(hipMemsetAsync(d.d_mp_ctr, 0, FZ_MP_CTR_WORDS * 8u, d.stream));
        if (ctx->timing) HIP_TRY(hipEventRecord(d.cur().ev[0], d.stream));
        hipLaunchKernelGGL(fk, dim3(grid), dim3(FZ_FILTER_THREADS), FZ_MP_FILTER_LDS, d.stream, sh.d_buf, a, ntiles, ddesc,
                           reinterpret_cast<uint64_t *>(d.d_mp_hits), dctr);
        HIP_TRY(hipGetLastError());
        if (ctx->timing) HIP_TRY(hipEventRecord(d.cur().ev[1], d.stream));
        // (rag: the shard is a batch — the ragged instances look every candidate's sequence up in the geometry's tables)
        if (cls)
            hipLaunchKernelGGL(rag ? fz_mp_batch_verify_cls_kernel : fz_mp_verify_cls_kernel, dim3((uint32_t)d.n_cus * 4), dim3(FZ_FILTER_THREADS),
                               fz_mp_verify_cls_lds(a.win_dwords), d.stream,
                               sh.d_buf, a, ddesc, reinterpret_cast<const uint64_t *>(d.d_mp_hits), reinterpret_cast<FzRec *>(d.d_mp_recs), dctr);
        else if (subs)
            hipLaunchKernelGGL(rag ? fz_mp_batch_verify_subs_kernel : fz_mp_verify_subs_kernel, dim3((uint32_t)d.n_cus * 4), dim3(FZ_FILTER_THREADS),
                               fz_mp_verify_subs_lds(a.win_dwords), d.stream,
                               sh.d_buf, a, ddesc, reinterpret_cast<const uint64_t *>(d.d_mp_hits), reinterpret_cast<FzRec *>(d.d_mp_recs), dctr);
        else
            hipLaunchKernelGGL(rag ? fz_mp_batch_verify_kernel : fz_mp_verify_kernel, dim3((uint32_t)d.n_cus * 4), dim3(FZ_FILTER_THREADS),
                               fz_mp_verify_lds(a.win_dwords), d.stream,
                               sh.d_buf, a, ddesc, reinterpret_cast<const uint64_t *>(d.d_mp_hits), reinterpret_cast<FzRec *>(d.d_mp_recs), dctr);
        HIP_TRY(hipGetLastError());
        if (ctx->timing) HIP_TRY(hipEventRecord(d.cur().ev[2], d.stream));
        unsigned long long ctr[FZ_MP_CTR_WORDS];
        HIP_TRY(hipMemcpyAsync(ctr, d.d_mp_ctr, sizeof ctr, hipMemcpyDeviceToHost, d.stream));
        HIP_TRY(hipStreamSynchronize(d.stream));
        ++tot.launches;
        if (ctx->timing) {
            tot.filter_ms += span_ms(d.cur().ev[0], d.cur().ev[1]);
            tot.verify_ms += span_ms(d.cur().ev[1], d.cur().ev[2]);
        }
        uint64_t need_hits = 0;
        for (uint32_t l = 0; l < FZ_MP_LISTS; ++l) need_hits = std::max<uint64_t>(need_hits, ctr[FZ_MP_CTR_LIST(l)]);
        const uint64_t nr = ctr[FZ_MP_CTR_RECS];
        if (need_hits > a.hit_cap || nr > a.rec_cap) {
            hit_cap = std::max(hit_cap, need_hits);
            // (records of a run whose hit lists were cut short are a lower bound: leave room for as many again)
            rec_cap = std::max(rec_cap, need_hits > a.hit_cap ? 2 * nr : nr);
            continue;
        }
        *n_recs = nr;
        uint64_t confirmed = 0, appended = 0;
        for (uint32_t i = 0; i < 64; ++i) confirmed += ctr[8 + i];
        for (uint32_t l = 0; l < FZ_MP_LISTS; ++l) appended += ctr[FZ_MP_CTR_LIST(l)];
        tot.hits += confirmed;
        if (sw().trace)
            fprintf(stderr, "[fz] multi group: %u blocks, %llu hits appended (%llu bytes written and read), %llu confirmed, %llu records\n",
                    nent, (unsigned long long)appended, (unsigned long long)(16 * appended), (unsigned long long)confirmed, (unsigned long long)nr);
        return FZ_OK;
    }
    return fail(FZ_EDEVICE, "result buffers kept overflowing");
}

// One group over one shard: its descriptor built (fz_mp_build), then mp_launch_shard.
// -> *n_recs records in d.d_mp_recs (aux = the pattern's number in the group), the stream idle.
static int mp_launch_group(fz_ctx *ctx, const Shard &sh, uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t k, const MpGroup &g,
                           uint64_t *n_recs, MpTotals &tot, bool rag, const MpCls *cls = nullptr) {
    const uint32_t np = (uint32_t)g.pats.size();
    const uint8_t *pp[FZ_MP_MAX_PATS];
    uint32_t pm[FZ_MP_MAX_PATS], max_m = 0;
    for (uint32_t j = 0; j < np; ++j) {
        pp[j] = pats + offs[g.pats[j]];
        pm[j] = (uint32_t)(offs[g.pats[j] + 1] - offs[g.pats[j]]);
        max_m = std::max(max_m, pm[j]);
    }
    std::vector<uint32_t> desc(cls ? FZ_MP_CLS_DESC_WORDS : FZ_MP_DESC_WORDS, 0u);
    const uint32_t nent = cls ? fz_mp_build_cls(desc.data(), pp, pm, np, g.L, cls->pmask, cls->tmask) : fz_mp_build(desc.data(), pp, pm, np, g.L);
    if (nent == 0 || nent != g.blocks) return fail(FZ_EDEVICE, "internal: the group's block table does not match its plan");
    return mp_launch_shard(ctx, sh, mode, desc.data(), nent, k, g.L, max_m, std::max(1u, mp_sigma(pats, offs, g)), n_recs, tot, rag, cls != nullptr);
}

// One group over every shard of the sequence, the records copied back -> rows[i] of every pattern i of the group.
static int mp_run_group(fz_ctx *ctx, fz_seq *seq, uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t k, const MpGroup &g,
                        std::vector<std::vector<fz_match>> &rows, MpTotals &tot, const MpCls *cls = nullptr) {
    const uint32_t np = (uint32_t)g.pats.size();
    std::vector<FzRec> recs;
    for (const Shard &sh : seq->shards) {
        uint64_t nr = 0;
        int rc = mp_launch_group(ctx, sh, mode, pats, offs, k, g, &nr, tot, seq->is_batch, cls);
        if (rc) return rc;
        const size_t at = recs.size();
        recs.resize(at + nr);
        if (nr) HIP_TRY(hipMemcpy(recs.data() + at, ctx->devs[sh.dev].d_mp_recs, nr * sizeof(FzRec), hipMemcpyDeviceToHost));
    }
    // per pattern: its records (aux = the pattern's number in the group) in the reference's order — block ascending, hit
    // index ascending, by the host ordering every search uses.  Shards own disjoint index ranges in global coordinates,
    // so the records of all shards are ordered together.
    std::vector<std::vector<FzRec>> per(np);
    for (const FzRec &r : recs) {
        if (r.aux >= np) return fail(FZ_EDEVICE, "internal: a record names pattern %u of a group of %u", r.aux, np);
        per[r.aux].push_back(r);
    }
    for (uint32_t j = 0; j < np; ++j) {
        for (FzRec &r : per[j]) r.aux = 0;
        int rc = emit_matches(per[j].data(), per[j].size(), g.L, nullptr, nullptr, 0, 0, false, &rows[g.pats[j]]);
        if (rc) return rc;
        tot.rows += rows[g.pats[j]].size();
    }
    return FZ_OK;
}

static int mp_check_lists(const uint8_t *pats, const uint64_t *offs, uint32_t n_pats) {
    if (n_pats && (!pats || !offs)) return fail(FZ_EINVAL, "null argument");
    for (uint32_t i = 0; i < n_pats; ++i)
        if (offs[i + 1] < offs[i]) return fail(FZ_EINVAL, "pattern offsets must not decrease");
    return FZ_OK;
}

// validate() accepts a batch handle inside a batch call only.
struct BatchScope {
    fz_ctx *c;
    explicit BatchScope(fz_ctx *c_) : c(c_) { c->batch_call = true; }
    ~BatchScope() { c->batch_call = false; }
};

// What every list-of-patterns call checks before anything is searched: the handles, the state of the context, the lists,
// and every pattern through the single call's checks (lev_plan / subs_plan).  batch_call: the name of a call that takes a
// batch handle (fz_batch_search_multi, fz_batch_assign), null for the calls of a whole sequence (fz_*_ngrams_multi*).
static int mp_admit(fz_ctx *ctx, fz_seq *seq, uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                    const char *batch_call) {
    if (!ctx || !seq || seq->ctx != ctx) return fail(FZ_EINVAL, "bad ctx/seq handle");
    if (batch_call) {
        if (mode != FZ_MODE_LEV && mode != FZ_MODE_SUBS) return fail(FZ_EINVAL, "mode must be Levenshtein or substitutions-only");
        int rc = batch_single_device(ctx, seq);
        if (rc) return rc;
        if (!seq->is_batch) return fail(FZ_EINVAL, "%s takes a batch handle (fz_batch_upload)", batch_call);
    } else if (seq->is_batch) {
        return fail(FZ_EINVAL, "a batch handle (fz_batch_upload) is searched with fz_batch_search only");
    }
    if (ctx->npend) return fail(FZ_EINVAL, "a search started with fz_lev_ngrams_begin is still in flight");
    if (ctx->stream_inflight) return fail(FZ_EINVAL, "a file stream of this context has a batch in flight (finish or close it first)");
    int rc = mp_check_lists(pats, offs, n_pats);
    if (rc) return rc;
    auto plans = [&]() {
        for (uint32_t i = 0; i < n_pats; ++i) {
            const uint64_t m = offs[i + 1] - offs[i];
            if (m > FZ_MAX_M_ANY) return fail(FZ_EUNSUPPORTED, "subsequence longer than %u bytes", FZ_MAX_M_ANY);
            Search q;
            int prc = mode == FZ_MODE_SUBS ? subs_plan(ctx, seq, m ? pats + offs[i] : nullptr, (uint32_t)m, k, q)
                                           : lev_plan(ctx, seq, m ? pats + offs[i] : nullptr, (uint32_t)m, k, q);
            if (prc) return prc;
        }
        return (int)FZ_OK;
    };
    if (!batch_call) return plans();
    BatchScope scope(ctx);
    return plans();
}

// The patterns outside every group, one search each: search(i, ran) runs pattern i as a single call and keeps what it
// found (ran = false: it had nothing to run); the stats that search left go into the totals, its verification form into
// `form` (form_none_too: also when the search verified nothing).
static int mp_run_solo(fz_ctx *ctx, const std::vector<uint32_t> &group_of, MpTotals &tot, uint32_t &form, bool form_none_too,
                       const std::function<int(uint32_t, bool &)> &search) {
    for (uint32_t i = 0; i < group_of.size(); ++i) {
        if (group_of[i] != 0xffffffffu) continue;
        bool ran = true;
        int rc = search(i, ran);
        if (rc) return rc;
        if (!ran) continue;
        tot.add_search(ctx->stats);
        if (form_none_too || ctx->stats.verify_form != FZ_FORM_NONE) form = ctx->stats.verify_form;
    }
    ctx->view = nullptr; ctx->view_n = 0; ctx->rows_ready = false;
    return FZ_OK;
}

// rows[i] (and, with seq_of, seq_in[i]: the sequence of every row) of n_pats patterns, back to back -> the call's result
// buffers; out_offs (optional): pattern i's rows are [offs[i], offs[i + 1]).  Nothing is left allocated on failure.
static int mp_pack(const std::vector<fz_match> *rows, const std::vector<uint32_t> *seq_in, uint32_t n_pats, fz_match **out, uint32_t **seq_of,
                   uint64_t **out_offs) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_pats; ++i) total += rows[i].size();
    void *mem = nullptr, *smem_ = nullptr, *omem = nullptr;
    int rc = alloc_out(total, sizeof(fz_match), &mem);
    if (rc == FZ_OK && seq_of) rc = alloc_out(total, sizeof(uint32_t), &smem_);
    if (rc == FZ_OK && out_offs) rc = alloc_out((uint64_t)n_pats + 1, sizeof(uint64_t), &omem);
    if (rc) { release_out(mem); release_out(smem_); release_out(omem); return rc; }
    fz_match *mo = static_cast<fz_match *>(mem);
    uint32_t *so = static_cast<uint32_t *>(smem_);
    uint64_t *oo = static_cast<uint64_t *>(omem);
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_pats; ++i) {
        if (oo) oo[i] = at;
        if (!rows[i].empty()) {
            memcpy(mo + at, rows[i].data(), rows[i].size() * sizeof(fz_match));
            if (so) memcpy(so + at, seq_in[i].data(), rows[i].size() * sizeof(uint32_t));
        }
        at += rows[i].size();
    }
    if (oo) oo[n_pats] = at;
    *out = mo;
    if (seq_of) *seq_of = so;
    if (out_offs) *out_offs = oo;
    return FZ_OK;
}

// What a call with classes plans with: mp_plan_cls' groups, or its refusal — before anything is searched.
static int mp_groups(uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k, const MpCls *cls,
                     std::vector<MpGroup> &groups, std::vector<uint32_t> &group_of) {
    if (cls) return mp_plan_cls(pats, offs, n_pats, k, *cls, groups, group_of);
    mp_plan(mode, pats, offs, n_pats, k, groups, group_of);
    return FZ_OK;
}

// fz_lev_ngrams_multi* (mode = FZ_MODE_LEV; reduced: fz_consolidate per pattern) and fz_subs_ngrams_multi* (FZ_MODE_SUBS;
// reduced: fz_group_best per pattern; cls: the class forms, every pattern on a pass).
static int multi_impl(fz_ctx *ctx, fz_seq *seq, uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                      bool consolidated, fz_match **out, uint64_t **out_offs, const MpCls *cls = nullptr) {
    const bool subs = mode == FZ_MODE_SUBS;
    if (!out || !out_offs) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *out_offs = nullptr;
    int rc = cls ? mp_check_cls(cls->pmask, cls->tmask) : (int)FZ_OK;
    if (rc) return rc;
    rc = mp_admit(ctx, seq, mode, pats, offs, n_pats, k, nullptr);
    if (rc) return rc;
    std::vector<MpGroup> groups;
    std::vector<uint32_t> group_of;
    // a context in a communicator searches collectively, pattern by pattern, through the existing collective search
    bool batched = !ctx->snapshot;
    for (const Shard &sh : seq->shards) batched = batched && sh.geom.seg_stride == 0;
    if (cls && !batched) return fail(FZ_EUNSUPPORTED, "symbol classes are searched on the multi-pattern pass only: not collectively, not over strided sequences");
    if (batched) rc = mp_groups(mode, pats, offs, n_pats, k, cls, groups, group_of);
    else group_of.assign(n_pats, 0xffffffffu);
    if (rc) return rc;
    std::vector<std::vector<fz_match>> rows(n_pats);
    MpTotals tot;
    uint32_t form = FZ_FORM_NONE;
    rc = mp_run_solo(ctx, group_of, tot, form, /* form_none_too = */ true, [&](uint32_t i, bool &ran) {
        fz_match *one = nullptr;
        uint64_t n_one = 0;
        const uint32_t m = (uint32_t)(offs[i + 1] - offs[i]);
        if (subs && seq->n < m) { ran = false; return (int)FZ_OK; }    // (fz_subs_ngrams answers before it searches: nothing to count)
        int src = subs ? fz_subs_ngrams(ctx, seq, pats + offs[i], m, k, &one, &n_one) : fz_lev_ngrams(ctx, seq, pats + offs[i], m, k, &one, &n_one);
        if (src) return src;
        rows[i].assign(one, one + n_one);
        release_out(one);
        tot.rows += n_one;
        return FZ_OK;
    });
    if (rc) return rc;
    for (const MpGroup &g : groups) {
        rc = mp_run_group(ctx, seq, mode, pats, offs, k, g, rows, tot, cls);
        if (rc) return rc;
        form = FZ_FORM_KERNEL;
    }
    if (consolidated) {
        for (uint32_t i = 0; i < n_pats; ++i) {
            fz_match *c = nullptr;
            uint64_t nc = 0;
            rc = subs ? fz_group_best(rows[i].data(), rows[i].size(), &c, &nc) : fz_consolidate(rows[i].data(), rows[i].size(), &c, &nc);
            if (rc) return rc;
            rows[i].assign(c, c + nc);
            release_out(c);
        }
    }
    rc = mp_pack(rows.data(), nullptr, n_pats, out, nullptr, out_offs);
    if (rc) return rc;
    mp_publish(ctx, tot, tot.rows, form);
    return FZ_OK;
}

int fz_lev_ngrams_multi(fz_ctx *ctx, fz_seq *seq, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                        fz_match **out, uint64_t **out_offs) {
    return multi_impl(ctx, seq, FZ_MODE_LEV, pats, offs, n_pats, k, false, out, out_offs);
}

int fz_lev_ngrams_multi_consolidated(fz_ctx *ctx, fz_seq *seq, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                                     fz_match **out, uint64_t **out_offs) {
    return multi_impl(ctx, seq, FZ_MODE_LEV, pats, offs, n_pats, k, true, out, out_offs);
}

int fz_subs_ngrams_multi(fz_ctx *ctx, fz_seq *seq, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                         fz_match **out, uint64_t **out_offs) {
    return multi_impl(ctx, seq, FZ_MODE_SUBS, pats, offs, n_pats, k, false, out, out_offs);
}

int fz_subs_ngrams_multi_best(fz_ctx *ctx, fz_seq *seq, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                              fz_match **out, uint64_t **out_offs) {
    return multi_impl(ctx, seq, FZ_MODE_SUBS, pats, offs, n_pats, k, true, out, out_offs);
}

int fz_subs_ngrams_multi_cls(fz_ctx *ctx, fz_seq *seq, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                             const uint8_t *pmask, const uint8_t *tmask, fz_match **out, uint64_t **out_offs) {
    const MpCls cls{pmask, tmask};
    return multi_impl(ctx, seq, FZ_MODE_SUBS, pats, offs, n_pats, k, false, out, out_offs, &cls);
}

int fz_subs_ngrams_multi_best_cls(fz_ctx *ctx, fz_seq *seq, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                                  const uint8_t *pmask, const uint8_t *tmask, fz_match **out, uint64_t **out_offs) {
    const MpCls cls{pmask, tmask};
    return multi_impl(ctx, seq, FZ_MODE_SUBS, pats, offs, n_pats, k, true, out, out_offs, &cls);
}

int fz_debug_multi_plan_cls(const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k, const uint8_t *pmask, const uint8_t *tmask,
                            uint32_t *group_of, uint32_t *n_groups, uint32_t *pat_entries, uint32_t *group_entries) {
    if (!group_of || !n_groups) return fail(FZ_EINVAL, "null argument");
    int rc = mp_check_cls(pmask, tmask);
    if (rc) return rc;
    rc = mp_check_lists(pats, offs, n_pats);
    if (rc) return rc;
    const MpCls cls{pmask, tmask};
    std::vector<MpGroup> groups;
    std::vector<uint32_t> of;
    rc = mp_plan_cls(pats, offs, n_pats, k, cls, groups, of, pat_entries);
    if (rc) return rc;
    for (uint32_t i = 0; i < n_pats; ++i) group_of[i] = of[i];
    if (group_entries)
        for (size_t gi = 0; gi < groups.size(); ++gi) group_entries[gi] = groups[gi].blocks;
    *n_groups = (uint32_t)groups.size();
    return FZ_OK;
}

int fz_debug_multi_plan(const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k, uint32_t *group_of, uint32_t *n_groups) {
    return fz_debug_multi_plan_mode(FZ_MODE_LEV, pats, offs, n_pats, k, group_of, n_groups);
}

int fz_debug_multi_plan_mode(uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k, uint32_t *group_of,
                             uint32_t *n_groups) {
    if (mode != FZ_MODE_LEV && mode != FZ_MODE_SUBS) return fail(FZ_EINVAL, "mode must be Levenshtein or substitutions-only");
    if (!group_of || !n_groups) return fail(FZ_EINVAL, "null argument");
    int rc = mp_check_lists(pats, offs, n_pats);
    if (rc) return rc;
    for (uint32_t i = 0; i < n_pats; ++i) {
        const uint64_t m = offs[i + 1] - offs[i];
        if (m == 0) return fail(FZ_EINVAL, "subsequence must not be empty");
        if (m > FZ_MAX_M_ANY) return fail(FZ_EUNSUPPORTED, "subsequence longer than %u bytes", FZ_MAX_M_ANY);
        if (m / ((uint64_t)k + 1) == 0) return fail(FZ_EINVAL, "the subsequence length must be greater than max_l_dist");
    }
    std::vector<MpGroup> groups;
    std::vector<uint32_t> of;
    mp_plan(mode, pats, offs, n_pats, k, groups, of);
    for (uint32_t i = 0; i < n_pats; ++i) group_of[i] = of[i];
    *n_groups = (uint32_t)groups.size();
    return FZ_OK;
}

// ... and of find_near_matches_generic_ngrams (generic_search.py:198-228).
static int generic_plan(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t max_subs, uint32_t max_ins, uint32_t max_dels,
                        uint32_t max_l, Search &q, bool in_pipeline = false) {
    int rc = validate(ctx, seq, p, m, in_pipeline);
    if (rc) return rc;
    const uint32_t k = max_l;
    if (k > FZ_MAX_K) return fail(FZ_EUNSUPPORTED, "max_l_dist above %d is not supported by the verify kernels", FZ_MAX_K);
    const uint32_t L = m / (k + 1);
    if (L == 0) return fail(FZ_EINVAL, "the subsequence length must be greater than max_l_dist");
    // the automaton's records carry window-relative start / end in 16 bits each: the window (m + 2k bytes) must fit
    if ((uint64_t)m + 2ull * k > 65535ull)
        return fail(FZ_EUNSUPPORTED, "generic search: len(subsequence) + 2 * max_l_dist = %llu exceeds 65535 (16-bit window coordinates)",
                    (unsigned long long)m + 2ull * k);
    rc = check_halo(seq, (uint64_t)m + k);
    if (rc) return rc;
    q.mode = FZ_MODE_GENERIC; q.m = m; q.k = k; q.p = p;
    q.max_subs = std::min(max_subs, 255u); q.max_ins = std::min(max_ins, 255u); q.max_dels = std::min(max_dels, 255u);
    q.plan.L = L;
    for (uint32_t s = 0; s + L <= m; s += L) q.plan.s.push_back(s);   // generic_search.py:221-228 (ranges: fz_block_range)
    if (q.plan.s.size() > FZ_MAX_BLOCKS) return fail(FZ_EUNSUPPORTED, "more than %u n-gram blocks", FZ_MAX_BLOCKS);
    return FZ_OK;
}

// What a finished generic search hands over: the raw stream in the reference's order, or — consolidated — the device's
// (hull, best match) pairs, one or a few per n-gram hit, through the second stage of the consolidation.
static int emit_generic_result(fz_ctx *ctx, fz_seq *seq, const Search &q, const std::vector<FzGenRec> &recs_vec, bool consolidated,
                               fz_match **out, uint64_t *n) {
    const uint32_t L = q.plan.L, k = q.k;
    if (!consolidated) return emit_generic(ctx, seq, recs_vec, L, k, out, n, nullptr);
    const FzGenRec *prs = ctx->gen_view ? ctx->gen_view : recs_vec.data();
    const size_t npr = ctx->gen_view ? (size_t)ctx->gen_view_n : recs_vec.size();
    static thread_local std::vector<Hull> hulls;
    hulls.clear();
    hulls.reserve(npr);
    for (size_t i = 0; i < npr; ++i) {
        const FzOutRow best = fz_gen_row(prs[i].key, L, k, 0, prs[i].se, prs[i].dist);
        const FzOutRow hull = fz_gen_row(prs[i].key, L, k, 0, prs[i].win, 0);
        hulls.push_back(Hull{hull.start, hull.end, fz_match{best.start, best.end, best.dist, best.block}});
    }
    ctx->stats.raw_matches = npr;
    return consolidate_hulls(hulls, out, n);
}

// Exchange step of a generic search in a one-process-per-GPU job: the automaton records (or folded pairs) of every rank,
// back to back; emit_generic / consolidate_hulls order them by their (block, index) keys, which are global.
static int generic_exchange(fz_ctx *ctx, std::vector<FzGenRec> &recs_vec) {
    if (!comm_multi_process(ctx)) return FZ_OK;
    const FzGenRec *mine = ctx->gen_view ? ctx->gen_view : recs_vec.data();
    const size_t nmine = ctx->gen_view ? (size_t)ctx->gen_view_n : recs_vec.size();
    std::vector<uint8_t> all;
    int rc = comm_gather_host(ctx, mine, nmine * sizeof(FzGenRec), all);
    if (rc) return rc;
    ctx->gen_view = nullptr;
    ctx->gen_view_n = 0;
    recs_vec.resize(all.size() / sizeof(FzGenRec));
    if (!all.empty()) memcpy(recs_vec.data(), all.data(), all.size());
    return FZ_OK;
}

static int pending_plan(fz_ctx *ctx, fz_ctx::Pending &pd, Search &q) {
    const uint8_t *p = pd.pattern.data();
    if (pd.kind == FZ_MODE_LEV) return lev_plan(ctx, pd.seq, p, pd.m, pd.k, q, true);
    if (pd.kind == FZ_MODE_SUBS) return subs_plan(ctx, pd.seq, p, pd.m, pd.k, q, true);
    int rc = generic_plan(ctx, pd.seq, p, pd.m, pd.max_subs, pd.max_ins, pd.max_dels, pd.k, q, true);
    q.fold = pd.consolidated;
    return rc;
}

// Launch a search and return (fz_lev_ngrams_begin, fz_subs_ngrams_begin, fz_generic_ngrams_begin); fz_search_end collects.
static int pending_begin(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t kind, uint32_t k, uint32_t max_subs,
                         uint32_t max_ins, uint32_t max_dels, bool consolidated) {
    if (ctx && ctx->npend >= 2) return fail(FZ_EINVAL, "two searches are already in flight on this context");
    const bool generic = kind == FZ_MODE_GENERIC;
    if (ctx && ctx->npend == 1 && (ctx->pend[0].kind == FZ_MODE_GENERIC) != generic)
        return fail(FZ_EINVAL, "generic searches and Levenshtein / substitutions-only searches cannot be in flight together");
    if (!ctx || !p || m == 0) return fail(FZ_EINVAL, "bad ctx / empty subsequence");
    fz_ctx::Pending &pd = ctx->pend[ctx->npend];
    pd.pattern.assign(p, p + m);                             // the caller's buffer is only borrowed for this call
    pd.seq = seq;
    pd.m = m;
    pd.k = k;
    pd.kind = kind;
    pd.max_subs = max_subs; pd.max_ins = max_ins; pd.max_dels = max_dels;
    pd.consolidated = consolidated;
    pd.lane = 0;
    Search q;
    int rc = pending_plan(ctx, pd, q);
    if (rc) return rc;
    memset(&ctx->stats, 0, sizeof ctx->stats); ctx->tref.clear();
    ctx->stats.n_devices = (uint32_t)ctx->devs.size();
    const bool second = ctx->npend == 1;
    pd.launched = true;
    if (generic) {
        // the lane the older search does not use; its scan then runs next to the older search's automaton kernel
        pd.lane = second ? 1 - ctx->pend[0].lane : 0;
        if (pd.lane == 1) { rc = ensure_lane2(ctx); if (rc) return rc; }
        std::vector<FzGenRec> none;
        ctx->lane = pd.lane;
        rc = run_generic(ctx, seq, q, none, /*phase=*/1);
        ctx->lane = 0;
        if (rc) return rc;
    } else {
        // with a search in flight this one goes to the devices' second result slot — unless a device is out of
        // direct mode (large record sets are fetched from the shared device buffer after the kernel: a second
        // search would overwrite it), then the launch waits for fz_search_end of the older search
        if (second && !ctx->snapshot) for (const DevState &d : ctx->devs) if (!d.direct || env_no_direct()) pd.launched = false;
        if (pd.launched) {
            if (second) for (DevState &d : ctx->devs) d.swap_slot();
            rc = search_enqueue(ctx, seq, q, true, /*behind=*/second);
            if (second) for (DevState &d : ctx->devs) d.swap_slot();
            if (rc) return rc;
        }
    }
    ++ctx->npend;
    return FZ_OK;
}

int fz_lev_ngrams_begin(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k) {
    return pending_begin(ctx, seq, p, m, FZ_MODE_LEV, k, 0, 0, 0, false);
}

int fz_subs_ngrams_begin(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k) {
    return pending_begin(ctx, seq, p, m, FZ_MODE_SUBS, k, 0, 0, 0, false);
}

int fz_generic_ngrams_begin(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t max_subs, uint32_t max_ins,
                            uint32_t max_dels, uint32_t max_l, int consolidated) {
    return pending_begin(ctx, seq, p, m, FZ_MODE_GENERIC, max_l, max_subs, max_ins, max_dels, consolidated != 0);
}

int fz_search_end(fz_ctx *ctx, fz_match **out, uint64_t *n) {
    if (!ctx || !out || !n) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *n = 0;
    if (!ctx->npend) return fail(FZ_EINVAL, "no search in flight");
    fz_ctx::Pending &pd = ctx->pend[0];
    Search q;
    int rc = pending_plan(ctx, pd, q);
    if (pd.kind == FZ_MODE_GENERIC) {
        std::vector<FzGenRec> recs_vec;
        ctx->lane = pd.lane;
        if (rc == FZ_OK) rc = run_generic(ctx, pd.seq, q, recs_vec, /*phase=*/2);
        if (rc == FZ_OK) rc = generic_exchange(ctx, recs_vec);
        if (rc == FZ_OK) rc = emit_generic_result(ctx, pd.seq, q, recs_vec, pd.consolidated, out, n);
        ctx->lane = 0;
        if (--ctx->npend == 1) std::swap(ctx->pend[0], ctx->pend[1]);
        if (rc != FZ_OK && *out) { release_out(*out); *out = nullptr; *n = 0; }
        return rc;
    }
    std::vector<FzRec> recs;
    std::vector<uint64_t> hits;
    if (rc == FZ_OK) rc = search_collect(ctx, pd.seq, q, true, recs, hits);
    if (rc == FZ_OK) rc = emit_matches(ctx, recs, q.plan.L, out, n, pd.seq->n, (uint32_t)q.plan.s.size());
    // the younger search (if any) becomes the oldest: its slot becomes the current one
    if (--ctx->npend == 1) {
        std::swap(ctx->pend[0], ctx->pend[1]);
        if (ctx->pend[0].launched) {
            for (DevState &d : ctx->devs) d.swap_slot();
        } else {                                             // deferred: launch it now, into the slot that just became free
            Search q2;
            int rc2 = pending_plan(ctx, ctx->pend[0], q2);
            if (rc2 == FZ_OK) rc2 = search_enqueue(ctx, ctx->pend[0].seq, q2, true);
            if (rc2 != FZ_OK) { ctx->npend = 0; if (rc == FZ_OK) rc = rc2; }
            ctx->pend[0].launched = true;
        }
    }
    if (rc != FZ_OK && *out) { release_out(*out); *out = nullptr; *n = 0; }   // an error never hands a buffer over
    return rc;
}

int fz_lev_ngrams_end(fz_ctx *ctx, fz_match **out, uint64_t *n) { return fz_search_end(ctx, out, n); }

// has_near_match_* stops at the first match (substitutions_only.py:218-233, generic_search.py:240-253).  On a long
// single-shard sequence the flag-only searches therefore scan the buffer in growing pieces — 64 MiB, then 4 x as much
// each time — and stop behind the first piece that produced a match: a match in the first MiB of 4 GiB costs one 64 MiB
// search (rounds 4 / 5: one launch whose not-yet-started workgroups skipped their tiles — a quarter of a full scan, bounded
// by the skipped workgroups' finish tickets; the generic form: a full scan + the automaton launch).  Without a match the
// pieces cost three more launches than one scan.  -> the byte ranges, or one whole-buffer range.
static std::vector<std::pair<uint64_t, uint64_t>> any_pieces(fz_ctx *ctx, fz_seq *seq) {
    std::vector<std::pair<uint64_t, uint64_t>> out;
    const uint64_t first = 64ull << 20;
    if (seq->shards.size() != 1 || comm_multi_process(ctx) || seq->shards[0].geom.seg_stride != 0 ||
        seq->shards[0].geom.buf_len < 8 * first) {
        out.emplace_back(0, ~0ull);
        return out;
    }
    const uint64_t len = seq->shards[0].geom.buf_len;
    uint64_t at = 0, size = first;
    while (at < len) {
        const uint64_t end = (len - at <= size + size / 2) ? len : at + size;      // (no sliver at the end)
        out.emplace_back(at, end >= len ? ~0ull : end);
        at = end;
        size *= 4;
    }
    return out;
}

static int subs_ngrams_impl(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, fz_match **out, uint64_t *n, int *found) {
    Search q;
    int rc = subs_plan(ctx, seq, p, m, k, q);
    if (rc) return rc;
    if (seq->n < m) return FZ_OK;                              // template :66-68
    const uint32_t L = q.plan.L;
    q.any = found != nullptr;
    if (q.any) q.collective = false;                           // a flag, not a stream: exchanged below
    std::vector<FzRec> recs;
    std::vector<uint64_t> hits;
    if (found) {
        bool any = false;
        for (const auto &piece : any_pieces(ctx, seq)) {
            q.part_lo = piece.first; q.part_hi = piece.second;
            rc = run_search(ctx, seq, q, true, recs, hits);
            if (rc) return rc;
            any = (ctx->view ? ctx->view_n : (uint64_t)recs.size()) > 0;
            if (any) break;
        }
        if (comm_multi_process(ctx)) { rc = comm_or(ctx, any); if (rc) return rc; }
        *found = any ? 1 : 0;
        return FZ_OK;
    }
    rc = run_search(ctx, seq, q, true, recs, hits);
    if (rc) return rc;
    return emit_matches(ctx, recs, L, out, n, seq->n, (uint32_t)q.plan.s.size());
}

int fz_subs_ngrams(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, fz_match **out, uint64_t *n) {
    if (!out || !n) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *n = 0;
    return subs_ngrams_impl(ctx, seq, p, m, k, out, n, nullptr);
}

// The substitutions-only n-gram search as the reference's wrapper returns it for bytes-like input (substitutions_only.py:
// 258-282): the best match of every overlap group in group-list order — fz_group_best of fz_subs_ngrams in one call.
int fz_subs_ngrams_best(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, fz_match **out, uint64_t *n) {
    if (!out || !n) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *n = 0;
    fz_match *raw = nullptr;
    uint64_t nraw = 0;
    int rc = subs_ngrams_impl(ctx, seq, p, m, k, &raw, &nraw, nullptr);
    if (rc) return rc;
    rc = fz_group_best(raw, nraw, out, n);
    release_out(raw);
    return rc;
}

int fz_subs_ngrams_any(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, int *found) {
    if (!found) return fail(FZ_EINVAL, "null argument");
    *found = 0;
    return subs_ngrams_impl(ctx, seq, p, m, k, nullptr, nullptr, found);
}

// Rows of the packed bytes in the in-memory order (block, index), global coordinates -> the batch's result: a row's
// sequence = the sequence of its first byte (a match lies inside the sequence of its n-gram hit); rows are ordered the way
// fz_stream_finish orders chunks: a stable sort by sequence of the in-memory order; local coordinates; `reduce`: every
// sequence's slice through fz_consolidate (Levenshtein) or fz_group_best.
static int batch_order(fz_seq *batch, uint32_t mode, bool reduce, const std::vector<fz_match> &rows, std::vector<fz_match> &fin,
                       std::vector<uint32_t> &fin_seq) {
    fin.clear();
    fin_seq.clear();
    const std::vector<uint64_t> &ends = batch->ends;
    std::vector<std::pair<uint32_t, uint32_t>> order(rows.size());       // (sequence, row)
    for (size_t i = 0; i < rows.size(); ++i) {
        const size_t j = (size_t)(std::upper_bound(ends.begin(), ends.end(), (uint64_t)rows[i].start) - ends.begin());
        if (j >= ends.size()) return fail(FZ_EDEVICE, "internal: a batch row outside every sequence");
        order[i] = {(uint32_t)j, (uint32_t)i};
    }
    if (rows.size() >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "more than 2^32 - 1 rows in a batch search");
    std::stable_sort(order.begin(), order.end(), [](const std::pair<uint32_t, uint32_t> &x, const std::pair<uint32_t, uint32_t> &y) { return x.first < y.first; });
    fin.reserve(rows.size());
    fin_seq.reserve(rows.size());
    std::vector<fz_match> slice;
    for (size_t a = 0; a < order.size();) {
        size_t b = a;
        const uint32_t j = order[a].first;
        const int64_t base = (int64_t)(j ? ends[j - 1] : 0);
        slice.clear();
        for (; b < order.size() && order[b].first == j; ++b) {
            fz_match r = rows[order[b].second];
            r.start -= base; r.end -= base;
            slice.push_back(r);
        }
        if (reduce) {
            fz_match *ro = nullptr;
            uint64_t rn = 0;
            int rc = mode == FZ_MODE_LEV ? fz_consolidate(slice.data(), slice.size(), &ro, &rn) : fz_group_best(slice.data(), slice.size(), &ro, &rn);
            if (rc) return rc;
            fin.insert(fin.end(), ro, ro + rn);
            fin_seq.insert(fin_seq.end(), rn, j);
            release_out(ro);
        } else {
            fin.insert(fin.end(), slice.begin(), slice.end());
            fin_seq.insert(fin_seq.end(), slice.size(), j);
        }
        a = b;
    }
    return FZ_OK;
}

// fz_batch_assign: the call's device state, and the fold of one launch's records into its tables.
struct AssignCall {
    DevState *d = nullptr;
    FzRagged rag{};
    uint64_t n = 0, n_seqs = 0;
    uint32_t k = 0;
    unsigned long long *d_lo = nullptr;
    uint32_t *d_hi = nullptr, *d_pm = nullptr;
    FzAssignRow *d_rows = nullptr;
    FzAssignPat *d_pat = nullptr;
    uint64_t folded = 0;
    double fold_ms = 0;
};

// The grid of the assignment's kernels: a lane per item, grid-stride beyond 8 workgroups per CU.
static uint32_t assign_grid(const DevState &d, uint64_t items) {
    return (uint32_t)std::min<uint64_t>((items + FZ_ASSIGN_THREADS - 1) / FZ_ASSIGN_THREADS, (uint64_t)d.n_cus * 8);
}

// launch() between ev[2] and ev[3] of a context that times its kernels; once ev[3] is complete the span goes to fold_ms.
static int assign_launch(fz_ctx *ctx, DevState &d, const std::function<void()> &launch) {
    if (ctx->timing) HIP_TRY(hipEventRecord(d.cur().ev[2], d.stream));
    launch();
    HIP_TRY(hipGetLastError());
    if (ctx->timing) HIP_TRY(hipEventRecord(d.cur().ev[3], d.stream));
    return FZ_OK;
}

// recs: n device records; table: npat entries of the call's aux table (one entry: aux ignored).  Stream-ordered, no wait.
static int assign_fold_device(fz_ctx *ctx, AssignCall &ac, const FzRec *d_recs, uint64_t n, uint32_t L, const FzAssignPat *table, uint32_t npat) {
    if (!n) return FZ_OK;
    DevState &d = *ac.d;
    int rc = assign_launch(ctx, d, [&]() {
        hipLaunchKernelGGL(fz_assign_reduce_kernel, dim3(assign_grid(d, n)), dim3(FZ_ASSIGN_THREADS), 0, d.stream, d_recs, n, L, ac.rag, ac.n,
                           table, npat, ac.k, ac.d_lo, ac.d_hi);
    });
    if (rc) return rc;
    if (ctx->timing) {
        HIP_TRY(hipEventSynchronize(d.cur().ev[3]));
        ac.fold_ms += span_ms(d.cur().ev[2], d.cur().ev[3]);
    }
    return FZ_OK;
}

// The records of a pattern searched on its own (host memory, empty slots included) -> the device -> the same fold.
static int assign_fold_host(fz_ctx *ctx, AssignCall &ac, const FzRec *recs, uint64_t n, uint32_t L, const FzAssignPat *table) {
    if (!n) return FZ_OK;
    DevState &d = *ac.d;
    HIP_TRY(hipSetDevice(d.device));
    if (d.assign_rec_cap < n) {
        const uint64_t cap = std::max<uint64_t>(n + n / 2, 4096);
        int rc = grow_device(d, d.d_assign_recs, d.assign_rec_cap, cap, cap * sizeof(FzRec));
        if (rc) return rc;
    }
    for (uint64_t i = 0; i < n; ++i) ac.folded += recs[i].dist != FZ_REC_NONE && recs[i].dist <= ac.k;
    HIP_TRY(hipMemcpyAsync(d.d_assign_recs, recs, (size_t)n * sizeof(FzRec), hipMemcpyHostToDevice, d.stream));
    int rc = assign_fold_device(ctx, ac, reinterpret_cast<const FzRec *>(d.d_assign_recs), n, L, table, 1u);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(d.stream));               // (the records are the search's own buffer, reused by the next one)
    return FZ_OK;
}

// fz_batch_search without its result buffers: what fz_batch_search_multi runs for the patterns outside every group.
// (assign / assign_table: fz_batch_assign — the search's records are folded where fz_batch_search would order them.)
static int batch_search_impl(fz_ctx *ctx, fz_seq *batch, uint32_t mode, const uint8_t *p, uint32_t m, uint32_t k, int reduced,
                             std::vector<fz_match> &fin, std::vector<uint32_t> &fin_seq, AssignCall *assign = nullptr,
                             const FzAssignPat *assign_table = nullptr) {
    if (!ctx || !batch || batch->ctx != ctx) return fail(FZ_EINVAL, "bad ctx/seq handle");
    if (mode != FZ_MODE_EXACT && mode != FZ_MODE_LEV && mode != FZ_MODE_SUBS) return fail(FZ_EINVAL, "mode must be exact, Levenshtein or substitutions-only");
    if (mode == FZ_MODE_EXACT && k != 0) return fail(FZ_EINVAL, "an exact search has no budget");
    BatchScope scope(ctx);
    Search q;
    int rc;
    if (mode == FZ_MODE_LEV) rc = lev_plan(ctx, batch, p, m, k, q);
    else if (mode == FZ_MODE_SUBS) rc = subs_plan(ctx, batch, p, m, k, q);
    else {
        rc = validate(ctx, batch, p, m);
        if (rc == FZ_OK) rc = check_halo(batch, m);
        q.mode = FZ_MODE_EXACT; q.m = m; q.k = 0; q.p = p;
        q.plan.L = m;
        q.plan.s = {0};
        q.plan.abs_lo = 0;
        q.plan.abs_hi = batch->n;
    }
    if (rc) return rc;
    rc = batch_single_device(ctx, batch);
    if (rc) return rc;
    q.collective = false;
    // the rows of the packed bytes in the in-memory order (block, index), global coordinates
    std::vector<fz_match> rows;
    memset(&ctx->stats, 0, sizeof ctx->stats);
    ctx->stats.n_devices = 1;
    if (batch->n_seqs && batch->n) {
        std::vector<FzRec> recs;
        std::vector<uint64_t> hits;
        rc = run_search(ctx, batch, q, mode != FZ_MODE_EXACT, recs, hits);
        if (rc) return rc;
        if (assign) {
            if (mode == FZ_MODE_EXACT || ctx->rows_ready) return fail(FZ_EDEVICE, "internal: no records to fold");
            return ctx->view ? assign_fold_host(ctx, *assign, ctx->view, ctx->view_n, q.plan.L, assign_table)
                             : assign_fold_host(ctx, *assign, recs.data(), recs.size(), q.plan.L, assign_table);
        }
        if (mode == FZ_MODE_EXACT) {
            std::sort(hits.begin(), hits.end());
            rows.resize(hits.size());
            for (size_t i = 0; i < hits.size(); ++i) {
                const int64_t at = (int64_t)fz_hit_index(hits[i]);
                rows[i].start = at; rows[i].end = at + m; rows[i].dist = 0; rows[i].block = -1;
            }
        } else {
            fz_match *mo = nullptr;
            uint64_t cnt = 0;
            rc = emit_matches(ctx, recs, q.plan.L, &mo, &cnt, batch->n, (uint32_t)q.plan.s.size());
            if (rc) return rc;
            rows.assign(mo, mo + cnt);
            release_out(mo);
        }
    }
    ctx->stats.raw_matches = rows.size();
    return batch_order(batch, mode, reduced != 0 && mode != FZ_MODE_EXACT, rows, fin, fin_seq);
}

int fz_batch_search(fz_ctx *ctx, fz_seq *batch, uint32_t mode, const uint8_t *p, uint32_t m, uint32_t k,
                    int reduced, fz_match **out, uint32_t **seq_of, uint64_t *n) {
    if (!out || !seq_of || !n) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *seq_of = nullptr; *n = 0;
    std::vector<fz_match> fin;
    std::vector<uint32_t> fin_seq;
    int rc = batch_search_impl(ctx, batch, mode, p, m, k, reduced, fin, fin_seq);
    if (rc) return rc;
    rc = mp_pack(&fin, &fin_seq, 1, out, seq_of, nullptr);
    if (rc) return rc;
    *n = fin.size();
    return FZ_OK;
}

// Many patterns over a batch: the multi-pattern planner (mp_plan, unchanged: fz_debug_multi_plan_mode answers for this call
// too), every group one filter launch over the packed bytes plus one RAGGED verification launch (fz_mp_batch_verify_kernel /
// fz_mp_batch_verify_subs_kernel: every candidate inside its own sequence), every other pattern through batch_search_impl.
// Per pattern the rows are then ordered, shifted and reduced exactly as fz_batch_search does it (batch_order).
static int batch_multi_impl(fz_ctx *ctx, fz_seq *batch, uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                            int reduced, fz_match **out, uint32_t **seq_of, uint64_t **out_offs, const MpCls *cls, const char *call) {
    if (!out || !seq_of || !out_offs) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *seq_of = nullptr; *out_offs = nullptr;
    int rc = cls ? mp_check_cls(cls->pmask, cls->tmask) : (int)FZ_OK;
    if (rc) return rc;
    rc = mp_admit(ctx, batch, mode, pats, offs, n_pats, k, call);
    if (rc) return rc;
    std::vector<MpGroup> groups;
    std::vector<uint32_t> group_of;
    rc = mp_groups(mode, pats, offs, n_pats, k, cls, groups, group_of);
    if (rc) return rc;
    std::vector<std::vector<fz_match>> fin(n_pats);
    std::vector<std::vector<uint32_t>> fin_seq(n_pats);
    MpTotals tot;
    uint32_t form = FZ_FORM_NONE;
    rc = mp_run_solo(ctx, group_of, tot, form, /* form_none_too = */ false, [&](uint32_t i, bool &) {
        int src = batch_search_impl(ctx, batch, mode, pats + offs[i], (uint32_t)(offs[i + 1] - offs[i]), k, reduced, fin[i], fin_seq[i]);
        if (src == FZ_OK) tot.rows += ctx->stats.raw_matches;
        return src;
    });
    if (rc) return rc;
    if (!groups.empty() && batch->n_seqs && batch->n) {
        std::vector<std::vector<fz_match>> rows(n_pats);           // global coordinates, in-memory order
        for (const MpGroup &g : groups) {
            rc = mp_run_group(ctx, batch, mode, pats, offs, k, g, rows, tot, cls);
            if (rc) return rc;
            form = FZ_FORM_KERNEL;
            for (uint32_t i : g.pats) {
                rc = batch_order(batch, mode, reduced != 0, rows[i], fin[i], fin_seq[i]);
                if (rc) return rc;
                std::vector<fz_match>().swap(rows[i]);
            }
        }
    }
    rc = mp_pack(fin.data(), fin_seq.data(), n_pats, out, seq_of, out_offs);
    if (rc) return rc;
    mp_publish(ctx, tot, tot.rows, form);
    return FZ_OK;
}

int fz_batch_search_multi(fz_ctx *ctx, fz_seq *batch, uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                          int reduced, fz_match **out, uint32_t **seq_of, uint64_t **out_offs) {
    return batch_multi_impl(ctx, batch, mode, pats, offs, n_pats, k, reduced, out, seq_of, out_offs, nullptr, "fz_batch_search_multi");
}

int fz_batch_search_multi_cls(fz_ctx *ctx, fz_seq *batch, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                              const uint8_t *pmask, const uint8_t *tmask, int reduced, fz_match **out, uint32_t **seq_of, uint64_t **out_offs) {
    const MpCls cls{pmask, tmask};
    return batch_multi_impl(ctx, batch, FZ_MODE_SUBS, pats, offs, n_pats, k, reduced, out, seq_of, out_offs, &cls, "fz_batch_search_multi_cls");
}

// Best pattern per sequence.  The checks, the plan and the launches of fz_batch_search_multi; behind every verification
// launch fz_assign_reduce_kernel folds the records where they lie into the call's tables (lo: u64, hi: u32 per sequence),
// fz_assign_finish_kernel decodes them and ONE copy brings the rows to the host: no record copy, no ordering, no rows.
static int batch_assign_impl(fz_ctx *ctx, fz_seq *batch, uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                             fz_assign **out, const MpCls *cls, const char *call) {
    static_assert(sizeof(fz_assign) == sizeof(FzAssignRow) && sizeof(fz_assign) == 16, "the kernel writes the C-ABI's rows");
    if (!out) return fail(FZ_EINVAL, "null argument");
    *out = nullptr;
    int rc = cls ? mp_check_cls(cls->pmask, cls->tmask) : (int)FZ_OK;
    if (rc) return rc;
    rc = mp_admit(ctx, batch, mode, pats, offs, n_pats, k, call);
    if (rc) return rc;
    std::vector<MpGroup> groups;
    std::vector<uint32_t> group_of;
    rc = mp_groups(mode, pats, offs, n_pats, k, cls, groups, group_of);      // (a class call's refusals: before anything is allocated)
    if (rc) return rc;
    // the domain of the tables' keys (fz_device.h: fz_assign_key)
    if (k > FZ_ASSIGN_MAX_K) return fail(FZ_EUNSUPPORTED, "best-pattern assignment takes budgets up to %u", FZ_ASSIGN_MAX_K);
    if (n_pats > FZ_ASSIGN_MAX_PATS) return fail(FZ_EUNSUPPORTED, "best-pattern assignment takes at most %u patterns", FZ_ASSIGN_MAX_PATS);
    if (batch->max_seq_len >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "best-pattern assignment takes sequences shorter than 2^32 bytes");
    const uint64_t n_seqs = batch->n_seqs;
    void *mem = nullptr;
    rc = alloc_out(n_seqs, sizeof(fz_assign), &mem);
    if (rc) return rc;
    struct Guard { void *p; ~Guard() { if (p) release_out(p); } } guard{mem};
    fz_assign *rows = static_cast<fz_assign *>(mem);
    ctx->view = nullptr; ctx->view_n = 0; ctx->rows_ready = false;
    mp_publish(ctx, MpTotals(), 0, FZ_FORM_NONE);
    if (n_pats == 0 || n_seqs == 0 || batch->n == 0) {         // nothing can match: nothing is launched
        for (uint64_t j = 0; j < n_seqs; ++j) { rows[j].pattern = -1; rows[j].dist = 0; rows[j].tied = 0; rows[j].start = 0; rows[j].end = 0; }
        guard.p = nullptr;
        *out = rows;
        return FZ_OK;
    }
    // the aux tables of the whole call: 64 entries per group, then one entry per pattern searched on its own
    std::vector<FzAssignPat> table(groups.size() * FZ_MP_MAX_PATS + n_pats);
    std::vector<uint32_t> pm(n_pats);
    for (uint32_t i = 0; i < n_pats; ++i) {
        pm[i] = (uint32_t)(offs[i + 1] - offs[i]);
        table[groups.size() * FZ_MP_MAX_PATS + i] = FzAssignPat{i, pm[i]};
    }
    for (size_t gi = 0; gi < groups.size(); ++gi)
        for (uint32_t j = 0; j < FZ_MP_MAX_PATS; ++j) {
            const uint32_t i = groups[gi].pats[j < groups[gi].pats.size() ? j : 0];
            table[gi * FZ_MP_MAX_PATS + j] = FzAssignPat{i, pm[i]};
        }
    const Shard &sh = batch->shards[0];
    DevState &d = ctx->devs[sh.dev];
    HIP_TRY(hipSetDevice(d.device));
    // lo | hi | rows | pattern lengths | aux tables (8-, 4-, 4-, 4-, 4-byte alignment; lo and hi are filled by one memset)
    const uint64_t o_hi = n_seqs * 8, o_rows = o_hi + n_seqs * 4, o_pm = o_rows + n_seqs * sizeof(FzAssignRow);
    const uint64_t o_pat = o_pm + (uint64_t)n_pats * 4, need = o_pat + table.size() * sizeof(FzAssignPat);
    rc = grow_device(d, d.d_assign, d.assign_cap, need, need);
    if (rc) return rc;
    AssignCall ac;
    ac.d = &d;
    ac.rag = fz_ragged(sh.geom);
    ac.n = sh.geom.n;
    ac.n_seqs = n_seqs;
    ac.k = k;
    ac.d_lo = reinterpret_cast<unsigned long long *>(d.d_assign);
    ac.d_hi = reinterpret_cast<uint32_t *>(d.d_assign + o_hi);
    ac.d_rows = reinterpret_cast<FzAssignRow *>(d.d_assign + o_rows);
    ac.d_pm = reinterpret_cast<uint32_t *>(d.d_assign + o_pm);
    ac.d_pat = reinterpret_cast<FzAssignPat *>(d.d_assign + o_pat);
    HIP_TRY(hipMemsetAsync(d.d_assign, 0xff, (size_t)o_rows, d.stream));
    HIP_TRY(hipMemcpyAsync(ac.d_pm, pm.data(), (size_t)n_pats * 4, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(ac.d_pat, table.data(), table.size() * sizeof(FzAssignPat), hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));               // (the searches below may run on the context's other stream)
    MpTotals tot;
    uint32_t form = FZ_FORM_NONE;
    std::vector<fz_match> no_rows;
    std::vector<uint32_t> no_seq;
    rc = mp_run_solo(ctx, group_of, tot, form, /* form_none_too = */ false, [&](uint32_t i, bool &) {
        return batch_search_impl(ctx, batch, mode, pats + offs[i], pm[i], k, 0, no_rows, no_seq, &ac, ac.d_pat + groups.size() * FZ_MP_MAX_PATS + i);
    });
    if (rc) return rc;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const MpGroup &g = groups[gi];
        uint64_t nr = 0;
        rc = mp_launch_group(ctx, sh, mode, pats, offs, k, g, &nr, tot, true, cls);
        if (rc) return rc;
        // the attempt that did not overflow: its records, where they lie
        rc = assign_fold_device(ctx, ac, reinterpret_cast<const FzRec *>(d.d_mp_recs), nr, g.L, ac.d_pat + gi * FZ_MP_MAX_PATS, FZ_MP_MAX_PATS);
        if (rc) return rc;
        ac.folded += nr;
        form = FZ_FORM_KERNEL;
    }
    rc = assign_launch(ctx, d, [&]() {
        hipLaunchKernelGGL(fz_assign_finish_kernel, dim3(assign_grid(d, n_seqs)), dim3(FZ_ASSIGN_THREADS), 0, d.stream, ac.d_lo, ac.d_hi, n_seqs,
                           ac.d_pm, k, ac.d_rows);
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(rows, ac.d_rows, (size_t)n_seqs * sizeof(fz_assign), hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    if (ctx->timing) ac.fold_ms += span_ms(d.cur().ev[2], d.cur().ev[3]);
    guard.p = nullptr;
    *out = rows;
    mp_publish(ctx, tot, ac.folded, form, ac.fold_ms);
    return FZ_OK;
}

int fz_batch_assign(fz_ctx *ctx, fz_seq *batch, uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                    fz_assign **out) {
    return batch_assign_impl(ctx, batch, mode, pats, offs, n_pats, k, out, nullptr, "fz_batch_assign");
}

int fz_batch_assign_cls(fz_ctx *ctx, fz_seq *batch, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                        const uint8_t *pmask, const uint8_t *tmask, fz_assign **out) {
    const MpCls cls{pmask, tmask};
    return batch_assign_impl(ctx, batch, FZ_MODE_SUBS, pats, offs, n_pats, k, out, &cls, "fz_batch_assign_cls");
}

int fz_debug_assign_fold(const uint64_t *offs, uint64_t n_seqs, const void *recs, uint64_t n, uint32_t L, const uint32_t *pat_table,
                         uint32_t n_table, const uint32_t *pat_m, uint32_t n_pats, uint32_t k, fz_assign *out) {
    if (!offs || !out || (n && !recs) || !pat_table || !n_table || (n_pats && !pat_m)) return fail(FZ_EINVAL, "null argument");
    if (n_seqs >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "more than 2^32 - 1 sequences in a batch");
    if (k > FZ_ASSIGN_MAX_K) return fail(FZ_EUNSUPPORTED, "best-pattern assignment takes budgets up to %u", FZ_ASSIGN_MAX_K);
    if (n_pats > FZ_ASSIGN_MAX_PATS) return fail(FZ_EUNSUPPORTED, "best-pattern assignment takes at most %u patterns", FZ_ASSIGN_MAX_PATS);
    for (uint64_t j = 0; j < n_seqs; ++j) {
        if (offs[j + 1] < offs[j]) return fail(FZ_EINVAL, "sequence offsets must not decrease");
        if (offs[j + 1] - offs[j] >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "best-pattern assignment takes sequences shorter than 2^32 bytes");
    }
    const FzAssignPat *table = reinterpret_cast<const FzAssignPat *>(pat_table);
    for (uint32_t i = 0; i < n_table; ++i)
        if (table[i].pattern >= n_pats) return fail(FZ_EINVAL, "the pattern table names pattern %u of %u", table[i].pattern, n_pats);
    const uint64_t total = offs[n_seqs];
    const uint64_t ntiles = (total + FZ_TILE_BYTES - 1) / FZ_TILE_BYTES;
    std::vector<uint32_t> first(ntiles + 1);
    fz_ragged_first(offs + 1, n_seqs, ntiles, first.data());
    FzRagged t;
    t.ends = offs + 1; t.first = first.data(); t.n_seqs = n_seqs;
    std::vector<uint64_t> lo(n_seqs, FZ_ASSIGN_NONE_LO);
    std::vector<uint32_t> hi(n_seqs, FZ_ASSIGN_NONE_HI);
    const uint8_t *rb = static_cast<const uint8_t *>(recs);
    for (uint64_t i = 0; i < n; ++i) {                        // the reduce kernel's lane, one record at a time
        FzRec r;
        memcpy(&r, rb + i * sizeof(FzRec), sizeof r);
        uint32_t seq, khi;
        uint64_t klo;
        if (!fz_assign_keys(t, total, r, L, table, n_table, k, seq, klo, khi)) continue;
        if (lo[seq] > klo) lo[seq] = klo;
        if (hi[seq] > khi) hi[seq] = khi;
    }
    for (uint64_t j = 0; j < n_seqs; ++j) {                   // the finish kernel's lane
        const FzAssignRow r = fz_assign_row(lo[j], hi[j], pat_m, k);
        memcpy(&out[j], &r, sizeof r);
    }
    return FZ_OK;
}

// ---------------------------------------------------------------------------------------------
// End overlaps (fz_batch_end_overlaps): per read the pattern whose strictly partial prefix ends it.  No filter, no plan: the
// list is cut into launches of fz_overlap_chunk patterns over ONE table of a key per read (fz_kernels.h: fz_overlap_kernel),
// the finish kernel decodes it and one copy brings the 8-byte rows back.

// What the call and its host twin refuse, in this order; then pm = the lengths and rows = the 64-byte rows of the patterns.
static int ovl_check(uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k, uint32_t min_overlap,
                     std::vector<uint32_t> &pm, std::vector<uint32_t> &rows) {
    if (mode != FZ_MODE_LEV && mode != FZ_MODE_SUBS) return fail(FZ_EUNSUPPORTED, "end overlaps: the mode must be Levenshtein or substitutions-only");
    if (int rc = mp_check_lists(pats, offs, n_pats)) return rc;
    if (min_overlap == 0) return fail(FZ_EINVAL, "end overlaps: min_overlap must be at least 1");
    if (n_pats > FZ_OVL_MAX_PATS) return fail(FZ_EUNSUPPORTED, "end overlaps take at most %u patterns", FZ_OVL_MAX_PATS);
    if (k > FZ_OVL_MAX_K) return fail(FZ_EUNSUPPORTED, "end overlaps take budgets up to %u", FZ_OVL_MAX_K);
    pm.assign(n_pats, 0u);
    rows.assign((size_t)n_pats * (FZ_OVL_ROW_BYTES / 4u), 0u);
    for (uint32_t i = 0; i < n_pats; ++i) {
        const uint64_t m = offs[i + 1] - offs[i];
        if (m == 0) return fail(FZ_EINVAL, "end overlaps: pattern %u is empty", i);
        if (m > FZ_OVL_MAX_M) return fail(FZ_EUNSUPPORTED, "end overlaps: pattern %u is longer than %u bytes", i, FZ_OVL_MAX_M);
        if (k >= m) return fail(FZ_EUNSUPPORTED, "end overlaps: pattern %u is not longer than the budget %u", i, k);
        pm[i] = (uint32_t)m;
        memcpy(reinterpret_cast<uint8_t *>(rows.data()) + (size_t)i * FZ_OVL_ROW_BYTES, pats + offs[i], (size_t)m);
    }
    return FZ_OK;
}

// The longest tail of the patterns [p0, p0 + npat).
static uint32_t ovl_tmax(uint32_t mode, const std::vector<uint32_t> &pm, uint32_t p0, uint32_t npat, uint32_t k) {
    uint32_t tmax = 0;
    for (uint32_t i = 0; i < npat; ++i) tmax = std::max(tmax, fz_overlap_tail(mode, pm[p0 + i], k));
    return tmax;
}

int fz_batch_end_overlaps(fz_ctx *ctx, fz_seq *batch, uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k,
                          uint32_t min_overlap, fz_overlap **out) {
    static_assert(sizeof(fz_overlap) == sizeof(FzOverlapRow) && sizeof(fz_overlap) == 8, "the kernel writes the C-ABI's rows");
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    if (!out) return fail(FZ_EINVAL, "null argument");
    *out = nullptr;
    if (!ctx || !batch || batch->ctx != ctx) return fail(FZ_EINVAL, "bad ctx/seq handle");
    std::vector<uint32_t> pm, prow;
    int rc = ovl_check(mode, pats, offs, n_pats, k, min_overlap, pm, prow);
    if (rc) return rc;
    if ((rc = batch_single_device(ctx, batch))) return rc;
    if (!batch->is_batch) return fail(FZ_EUNSUPPORTED, "fz_batch_end_overlaps takes a batch handle (fz_batch_upload)");
    if (ctx->npend || ctx->stream_inflight) return fail(FZ_EINVAL, "a search of this context is in flight");
    if (batch->max_seq_len >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "end overlaps take sequences shorter than 2^32 bytes");
    const uint64_t n_seqs = batch->n_seqs;
    void *mem = nullptr;
    if ((rc = alloc_out(n_seqs, sizeof(fz_overlap), &mem))) return rc;
    struct Guard { void *p; ~Guard() { if (p) release_out(p); } } guard{mem};
    fz_overlap *res = static_cast<fz_overlap *>(mem);
    ctx->view = nullptr; ctx->view_n = 0; ctx->rows_ready = false;
    mp_publish(ctx, MpTotals(), 0, FZ_FORM_NONE);
    for (double &ms : ctx->ovl_ms) ms = 0;
    if (n_pats == 0 || n_seqs == 0 || batch->n == 0) {         // nothing can overlap: nothing is launched
        for (uint64_t j = 0; j < n_seqs; ++j) {
            const FzOverlapRow r = fz_overlap_row(0ull, (uint32_t)(batch->ends[j] - (j ? batch->ends[j - 1] : 0ull)));
            memcpy(&res[j], &r, sizeof r);
        }
        guard.p = nullptr;
        *out = res;
        ctx->ovl_ms[3] = since(t_call);
        return FZ_OK;
    }
    const Shard &sh = batch->shards[0];
    DevState &d = ctx->devs[sh.dev];
    HIP_TRY(hipSetDevice(d.device));
    // table | rows | pattern lengths | pattern rows (8-, 8-, 4-, 4-byte alignment)
    const uint64_t o_rows = n_seqs * 8, o_pm = o_rows + n_seqs * sizeof(FzOverlapRow), o_pat = o_pm + (uint64_t)n_pats * 4;
    const uint64_t need = o_pat + (uint64_t)n_pats * FZ_OVL_ROW_BYTES;
    if ((rc = grow_device(d, d.d_assign, d.assign_cap, need, need))) return rc;
    unsigned long long *d_table = reinterpret_cast<unsigned long long *>(d.d_assign);
    FzOverlapRow *d_rows = reinterpret_cast<FzOverlapRow *>(d.d_assign + o_rows);
    const auto t_h2d = std::chrono::steady_clock::now();
    HIP_TRY(hipMemsetAsync(d_table, 0, (size_t)o_rows, d.stream));
    HIP_TRY(hipMemcpyAsync(d.d_assign + o_pm, pm.data(), (size_t)n_pats * 4, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(d.d_assign + o_pat, prow.data(), (size_t)n_pats * FZ_OVL_ROW_BYTES, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));               // (pm and prow are the call's own: the copies are done before they go)
    ctx->ovl_ms[0] = since(t_h2d);
    FzOvlArgs a;
    a.rag = fz_ragged(sh.geom);
    a.buf_len = sh.geom.buf_len;
    a.rows = reinterpret_cast<const uint32_t *>(d.d_assign + o_pat);
    a.pm = reinterpret_cast<const uint32_t *>(d.d_assign + o_pm);
    a.k = k; a.o = min_overlap;
    MpTotals tot;
    const uint32_t chunk = fz_overlap_chunk(mode);
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n_seqs + FZ_FILTER_THREADS - 1) / FZ_FILTER_THREADS, (uint64_t)d.n_cus * 8);
    if (ctx->timing) HIP_TRY(hipEventRecord(d.cur().ev[2], d.stream));
    for (uint32_t p0 = 0; p0 < n_pats; p0 += chunk) {
        a.p0 = p0;
        a.npat = std::min(chunk, n_pats - p0);
        a.tmax = ovl_tmax(mode, pm, p0, a.npat, k);
        a.win_dwords = fz_overlap_win_dwords(a.tmax);
        const uint32_t lds = fz_overlap_lds(mode, a.npat, a.win_dwords);
        if (mode == FZ_MODE_LEV)
            hipLaunchKernelGGL(fz_overlap_kernel<FZ_MODE_LEV>, dim3(grid), dim3(FZ_FILTER_THREADS), lds, d.stream, sh.d_buf, a, d_table);
        else
            hipLaunchKernelGGL(fz_overlap_kernel<FZ_MODE_SUBS>, dim3(grid), dim3(FZ_FILTER_THREADS), lds, d.stream, sh.d_buf, a, d_table);
        HIP_TRY(hipGetLastError());
        ++tot.launches;
    }
    hipLaunchKernelGGL(fz_overlap_finish_kernel, dim3(assign_grid(d, n_seqs)), dim3(FZ_ASSIGN_THREADS), 0, d.stream, d_table, a.rag.ends, n_seqs, d_rows);
    HIP_TRY(hipGetLastError());
    if (ctx->timing) HIP_TRY(hipEventRecord(d.cur().ev[3], d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    const auto t_d2h = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpyAsync(res, d_rows, (size_t)n_seqs * sizeof(fz_overlap), hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    ctx->ovl_ms[2] = since(t_d2h);
    if (ctx->timing) ctx->ovl_ms[1] = span_ms(d.cur().ev[2], d.cur().ev[3]);
    tot.bytes = sh.geom.buf_len;
    guard.p = nullptr;
    *out = res;
    mp_publish(ctx, tot, 0, FZ_FORM_NONE, ctx->ovl_ms[1]);
    ctx->ovl_ms[3] = since(t_call);
    return FZ_OK;
}

int fz_debug_overlap_ms(fz_ctx *ctx, double *ms4) {
    if (!ctx || !ms4) return fail(FZ_EINVAL, "null argument");
    for (int i = 0; i < 4; ++i) ms4[i] = ctx->ovl_ms[i];
    return FZ_OK;
}

int fz_debug_end_overlaps(uint32_t mode, const uint8_t *pats, const uint64_t *offs, uint32_t n_pats, uint32_t k, uint32_t min_overlap,
                          const uint8_t *bytes, const uint64_t *ends, uint64_t n_seqs, fz_overlap *out) {
    if ((n_seqs && (!ends || !out)) || (n_seqs && ends[n_seqs - 1] && !bytes)) return fail(FZ_EINVAL, "null argument");
    std::vector<uint32_t> pm, prow;
    if (int rc = ovl_check(mode, pats, offs, n_pats, k, min_overlap, pm, prow)) return rc;
    if (n_seqs >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "more than 2^32 - 1 sequences in a batch");
    for (uint64_t j = 0; j < n_seqs; ++j) {
        const uint64_t sa = j ? ends[j - 1] : 0ull;
        if (ends[j] < sa) return fail(FZ_EINVAL, "sequence offsets must not decrease");
        if (ends[j] - sa >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "end overlaps take sequences shorter than 2^32 bytes");
    }
    const uint64_t total = n_seqs ? ends[n_seqs - 1] : 0ull;
    std::vector<uint8_t> buf((total + 3u) & ~(uint64_t)3, 0);  // the device's buffer: zeros behind the data
    if (total) memcpy(buf.data(), bytes, (size_t)total);
    std::vector<uint64_t> table(n_seqs, 0ull);
    const uint32_t chunk = fz_overlap_chunk(mode);
    std::vector<uint64_t> peq;
    std::vector<uint32_t> win;
    for (uint32_t p0 = 0; p0 < n_pats; p0 += chunk) {         // one launch
        const uint32_t npat = std::min(chunk, n_pats - p0), tmax = ovl_tmax(mode, pm, p0, npat, k), win_dwords = fz_overlap_win_dwords(tmax);
        const uint32_t *rows = prow.data() + (size_t)p0 * (FZ_OVL_ROW_BYTES / 4u);
        peq.assign(mode == FZ_MODE_LEV ? (size_t)npat * 512u : 0u, 0ull);
        for (size_t i = 0; i < peq.size(); ++i)
            peq[i] = fz_overlap_peq_word(reinterpret_cast<const uint8_t *>(rows + (i >> 9) * (FZ_OVL_ROW_BYTES / 4u)), pm[p0 + (i >> 9)], i & 255u, (i >> 8) & 1u);
        const FzOvlTabs tb{pm.data() + p0, rows, peq.data()};
        win.assign(win_dwords, 0u);
        for (uint64_t j = 0; j < n_seqs; ++j) {               // one lane
            const uint64_t sa = j ? ends[j - 1] : 0ull, se = ends[j];
            const FzOvlStage st = fz_overlap_stage(sa, se, tmax, total);
            fz_overlap_stage_copy(buf.data(), st, win_dwords, win.data(), 1u);
            const uint64_t key = mode == FZ_MODE_LEV ? fz_overlap_lane<FZ_MODE_LEV>(tb, win.data(), 1u, st, (uint32_t)(se - sa), p0, npat, k, min_overlap)
                                                     : fz_overlap_lane<FZ_MODE_SUBS>(tb, win.data(), 1u, st, (uint32_t)(se - sa), p0, npat, k, min_overlap);
            table[j] = std::max(table[j], key);
        }
    }
    for (uint64_t j = 0; j < n_seqs; ++j) {                   // the finish kernel's lane
        const FzOverlapRow r = fz_overlap_row(table[j], (uint32_t)(ends[j] - (j ? ends[j - 1] : 0ull)));
        memcpy(&out[j], &r, sizeof r);
    }
    return FZ_OK;
}

// ---------------------------------------------------------------------------------------------
// Score cuts (fz_batch_score_cuts): per read where the running sum of a score table, taken from its 3' and / or its 5' end,
// peaks.  One launch (fz_kernels.h: fz_cuts_kernel), the lanes write the 8-byte rows, one copy brings them back.

// The call's tables as the kernel takes them: side s (0: 3', 1: 5') at w + 256 s, zeros for a side not asked for.
struct CutPlan {
    int16_t w[512];
    uint32_t sides = 0, walk = 0;                // asked for; asked for with a positive score in the table
    int32_t wmax[2] = {0, 0};
    uint32_t wabs = 0;                           // the largest |score| of the tables asked for
};

// What the call and its host twin refuse first, in this order.
static int cut_check(const int16_t *w3, const int16_t *w5, uint32_t flags, uint32_t rate_den, CutPlan &p) {
    if (!w3 && !w5) return fail(FZ_EINVAL, "score cuts: no table, w3 and w5 are both null");
    if (flags & ~(FZ_CUT_STOP3 | FZ_CUT_STOP5 | FZ_CUT_RATE)) return fail(FZ_EINVAL, "score cuts: flags 0x%x outside FZ_CUT_STOP3 | FZ_CUT_STOP5 | FZ_CUT_RATE", flags);
    if ((flags & FZ_CUT_RATE) && rate_den == 0) return fail(FZ_EINVAL, "score cuts: rate_den must not be 0 with FZ_CUT_RATE");
    memset(p.w, 0, sizeof p.w);
    const int16_t *tabs[2] = {w3, w5};
    for (uint32_t side = 0; side < 2; ++side) {
        if (!tabs[side]) continue;
        memcpy(p.w + 256 * side, tabs[side], 512);
        int32_t hi = -32768;
        for (uint32_t c = 0; c < 256; ++c) {
            const int32_t v = tabs[side][c];
            hi = std::max(hi, v);
            p.wabs = std::max(p.wabs, (uint32_t)(v < 0 ? -v : v));
        }
        p.wmax[side] = hi;
        p.sides |= 1u << side;
        if (hi > 0) p.walk |= 1u << side;
    }
    return FZ_OK;
}

// ... and last: what keeps the lanes' 32-bit sums from wrapping.
static int cut_check_sums(uint64_t max_seq_len, const CutPlan &p) {
    if (max_seq_len >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "score cuts take sequences shorter than 2^32 bytes");
    if (max_seq_len * p.wabs >= (1ull << 31))
        return fail(FZ_EUNSUPPORTED, "score cuts: the longest sequence (%llu bytes) times the largest |score| (%u) is not below 2^31",
                    (unsigned long long)max_seq_len, p.wabs);
    return FZ_OK;
}

int fz_batch_score_cuts(fz_ctx *ctx, fz_seq *batch, const int16_t *w3, const int16_t *w5, uint32_t flags, uint32_t rate_num,
                        uint32_t rate_den, fz_cut **out) {
    static_assert(sizeof(fz_cut) == sizeof(FzCutRow) && sizeof(fz_cut) == 8, "the kernel writes the C-ABI's rows");
    const auto t_call = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    if (!out) return fail(FZ_EINVAL, "null argument");
    *out = nullptr;
    if (!ctx || !batch || batch->ctx != ctx) return fail(FZ_EINVAL, "bad ctx/seq handle");
    CutPlan p;
    int rc = cut_check(w3, w5, flags, rate_den, p);
    if (rc) return rc;
    if ((rc = batch_single_device(ctx, batch))) return rc;
    if (!batch->is_batch) return fail(FZ_EUNSUPPORTED, "fz_batch_score_cuts takes a batch handle (fz_batch_upload)");
    if (ctx->npend || ctx->stream_inflight) return fail(FZ_EINVAL, "a search of this context is in flight");
    if ((rc = cut_check_sums(batch->max_seq_len, p))) return rc;
    const uint64_t n_seqs = batch->n_seqs;
    void *mem = nullptr;
    if ((rc = alloc_out(n_seqs, sizeof(fz_cut), &mem))) return rc;
    struct Guard { void *p; ~Guard() { if (p) release_out(p); } } guard{mem};
    fz_cut *res = static_cast<fz_cut *>(mem);
    ctx->view = nullptr; ctx->view_n = 0; ctx->rows_ready = false;
    mp_publish(ctx, MpTotals(), 0, FZ_FORM_NONE);
    for (double &ms : ctx->cut_ms) ms = 0;
    if (p.walk == 0 || n_seqs == 0 || batch->n == 0) {        // nothing can be cut: nothing is launched
        for (uint64_t j = 0; j < n_seqs; ++j) {
            const FzCutRow r = fz_cuts_row((uint32_t)(batch->ends[j] - (j ? batch->ends[j - 1] : 0ull)), 0u, 0u, p.sides);
            memcpy(&res[j], &r, sizeof r);
        }
        guard.p = nullptr;
        *out = res;
        ctx->cut_ms[3] = since(t_call);
        return FZ_OK;
    }
    const Shard &sh = batch->shards[0];
    DevState &d = ctx->devs[sh.dev];
    HIP_TRY(hipSetDevice(d.device));
    // rows | tables (8-, 2-byte alignment)
    const uint64_t o_tab = n_seqs * sizeof(FzCutRow), need = o_tab + sizeof p.w;
    if ((rc = grow_device(d, d.d_assign, d.assign_cap, need, need))) return rc;
    FzCutRow *d_rows = reinterpret_cast<FzCutRow *>(d.d_assign);
    const auto t_h2d = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpyAsync(d.d_assign + o_tab, p.w, sizeof p.w, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));               // (p is the call's own: the copy is done before it goes)
    ctx->cut_ms[0] = since(t_h2d);
    FzCutArgs a;
    a.rag = fz_ragged(sh.geom);
    a.buf_len = sh.geom.buf_len;
    a.w = reinterpret_cast<const int16_t *>(d.d_assign + o_tab);
    a.sides = p.sides; a.walk = p.walk; a.flags = flags;
    a.num = rate_num; a.den = rate_den;
    a.wmax3 = p.wmax[0]; a.wmax5 = p.wmax[1];
    MpTotals tot;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n_seqs + FZ_FILTER_THREADS - 1) / FZ_FILTER_THREADS, (uint64_t)d.n_cus * 8);
    if (ctx->timing) HIP_TRY(hipEventRecord(d.cur().ev[2], d.stream));
    hipLaunchKernelGGL(fz_cuts_kernel, dim3(grid), dim3(FZ_FILTER_THREADS), 0, d.stream, sh.d_buf, a, d_rows);
    HIP_TRY(hipGetLastError());
    ++tot.launches;
    if (ctx->timing) HIP_TRY(hipEventRecord(d.cur().ev[3], d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    const auto t_d2h = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpyAsync(res, d_rows, (size_t)n_seqs * sizeof(fz_cut), hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    ctx->cut_ms[2] = since(t_d2h);
    if (ctx->timing) ctx->cut_ms[1] = span_ms(d.cur().ev[2], d.cur().ev[3]);
    tot.bytes = sh.geom.buf_len;
    guard.p = nullptr;
    *out = res;
    mp_publish(ctx, tot, 0, FZ_FORM_NONE, ctx->cut_ms[1]);
    ctx->cut_ms[3] = since(t_call);
    return FZ_OK;
}

int fz_debug_cuts_ms(fz_ctx *ctx, double *ms4) {
    if (!ctx || !ms4) return fail(FZ_EINVAL, "null argument");
    for (int i = 0; i < 4; ++i) ms4[i] = ctx->cut_ms[i];
    return FZ_OK;
}

int fz_debug_score_cuts(const int16_t *w3, const int16_t *w5, uint32_t flags, uint32_t rate_num, uint32_t rate_den,
                        const uint8_t *bytes, const uint64_t *ends, uint64_t n_seqs, fz_cut *out) {
    if ((n_seqs && (!ends || !out)) || (n_seqs && ends[n_seqs - 1] && !bytes)) return fail(FZ_EINVAL, "null argument");
    CutPlan p;
    if (int rc = cut_check(w3, w5, flags, rate_den, p)) return rc;
    if (n_seqs >= (1ull << 32)) return fail(FZ_EUNSUPPORTED, "more than 2^32 - 1 sequences in a batch");
    uint64_t longest = 0;
    for (uint64_t j = 0; j < n_seqs; ++j) {
        const uint64_t sa = j ? ends[j - 1] : 0ull;
        if (ends[j] < sa) return fail(FZ_EINVAL, "sequence offsets must not decrease");
        longest = std::max(longest, ends[j] - sa);
    }
    if (int rc = cut_check_sums(longest, p)) return rc;
    const uint64_t total = n_seqs ? ends[n_seqs - 1] : 0ull;
    std::vector<uint8_t> buf((total + 3u) & ~(uint64_t)3, 0);  // the device's buffer: zeros behind the data
    if (total) memcpy(buf.data(), bytes, (size_t)total);
    uint32_t win[FZ_CUT_PIECE_DWORDS];
    for (uint64_t j = 0; j < n_seqs; ++j) {                   // one lane
        const uint64_t sa = j ? ends[j - 1] : 0ull, se = ends[j];
        const uint32_t n = (uint32_t)(se - sa);
        uint32_t trim[2] = {0u, 0u};
        for (uint32_t side = 0; side < 2u; ++side) {
            if (!((p.walk >> side) & 1u)) continue;
            const FzCutRule r = fz_cuts_rule(side, flags, rate_num, rate_den, p.wmax[side], 1u);
            FzCutState c = fz_cuts_begin(n, r);
            while (c.live) {                                  // one piece
                const FzOvlStage st = fz_cuts_piece(c, sa, se, side, total);
                fz_stage_copy<false>(buf.data(), st, FZ_CUT_PIECE_DWORDS, win, 1u);
                fz_cuts_lane(c, p.w + 256 * side, win, 1u, st, n, side, r);
            }
            trim[side] = c.trim;
        }
        const FzCutRow row = fz_cuts_row(n, trim[0], trim[1], p.sides);
        memcpy(&out[j], &row, sizeof row);
    }
    return FZ_OK;
}

static int generic_ngrams_impl(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t max_subs, uint32_t max_ins,
                               uint32_t max_dels, uint32_t max_l, fz_match **out, uint64_t *n, int *found, bool consolidated = false) {
    Search q;
    int rc = generic_plan(ctx, seq, p, m, max_subs, max_ins, max_dels, max_l, q);
    if (rc) return rc;
    q.any = found != nullptr;
    q.fold = consolidated;
    std::vector<FzGenRec> recs_vec;
    Trace tr;
    if (found) {
        bool any = false;
        for (const auto &piece : any_pieces(ctx, seq)) {       // (the scan of a piece lists its hits, the automaton runs on them)
            q.part_lo = piece.first; q.part_hi = piece.second;
            rc = run_generic(ctx, seq, q, recs_vec);
            if (rc) return rc;
            any = ctx->any_found;
            if (any) break;
        }
        if (comm_multi_process(ctx)) { rc = comm_or(ctx, any); if (rc) return rc; }
        *found = any ? 1 : 0;
        return FZ_OK;
    }
    rc = run_generic(ctx, seq, q, recs_vec);
    if (rc) return rc;
    tr.mark("generic: kernels");
    rc = generic_exchange(ctx, recs_vec);
    if (rc) return rc;
    rc = emit_generic_result(ctx, seq, q, recs_vec, consolidated, out, n);
    tr.mark("generic: rows");
    return rc;
}

int fz_generic_ngrams_consolidated(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t max_subs, uint32_t max_ins,
                                   uint32_t max_dels, uint32_t max_l, fz_match **out, uint64_t *n) {
    if (!out || !n) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *n = 0;
    return generic_ngrams_impl(ctx, seq, p, m, max_subs, max_ins, max_dels, max_l, out, n, nullptr, true);
}

int fz_generic_ngrams(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t max_subs, uint32_t max_ins,
                      uint32_t max_dels, uint32_t max_l, fz_match **out, uint64_t *n) {
    if (!out || !n) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *n = 0;
    return generic_ngrams_impl(ctx, seq, p, m, max_subs, max_ins, max_dels, max_l, out, n, nullptr);
}

int fz_generic_ngrams_any(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t max_subs, uint32_t max_ins,
                          uint32_t max_dels, uint32_t max_l, int *found) {
    if (!found) return fail(FZ_EINVAL, "null argument");
    *found = 0;
    return generic_ngrams_impl(ctx, seq, p, m, max_subs, max_ins, max_dels, max_l, nullptr, nullptr, found);
}

}  // extern "C"

namespace {

// Reference order: (segment,) hits in (block, idx) order, each hit's matches in automaton emission order.
// A wave writes the matches of its hit in contiguous runs (one bulk append per <= 512 matches) that
// are already in emission order, so only the runs are ordered, by (segment, key, first emission number),
// and the 24-byte records are read once: 2.1e5 records order in ~0.4 ms instead of ~2 ms.
int emit_generic(fz_ctx *ctx, fz_seq *seq, const std::vector<FzGenRec> &recs_vec, uint32_t L, uint32_t k, fz_match **out,
                 uint64_t *n, uint32_t **seg_out) {
    if (ctx->gen_rows_dev) {                                   // ordered and finished on the device: one copy
        static_assert(sizeof(FzOutRow) == sizeof(fz_match) && offsetof(FzOutRow, dist) == offsetof(fz_match, dist) &&
                      offsetof(FzOutRow, block) == offsetof(fz_match, block), "FzOutRow is fz_match");
        const uint64_t nrows = ctx->gen_rows_n;
        HIP_TRY(hipSetDevice(ctx->gen_rows_device));
        void *mem = nullptr;
        int rc = alloc_out(nrows, sizeof(fz_match), &mem);
        if (rc) return rc;
        hipError_t e = hipMemcpy(mem, ctx->gen_rows_dev, nrows * sizeof(fz_match), hipMemcpyDeviceToHost);
        if (e != hipSuccess) { release_out(mem); return fail(FZ_EDEVICE, "hipMemcpy of the ordered rows: %s", hipGetErrorString(e)); }
        if (seg_out) *seg_out = nullptr;
        *out = static_cast<fz_match *>(mem);
        *n = nrows;
        ctx->stats.raw_matches = nrows;
        return FZ_OK;
    }
    struct Run { uint64_t key; uint32_t seg; uint32_t seq0; uint32_t len; size_t first; };
    std::vector<Run> runs;
    const FzGeom &geom = seq->shards.empty() ? FzGeom{} : seq->shards[0].geom;
    const bool segs = geom.seg_stride != 0;                    // without segments `win` is the hit's slot, not a segment
    const FzGenRec *recs = ctx->gen_view ? ctx->gen_view : recs_vec.data();
    const size_t nrecs = ctx->gen_view ? (size_t)ctx->gen_view_n : recs_vec.size();
    for (size_t i = 0; i < nrecs;) {
        size_t j = i + 1;
        while (j < nrecs && recs[j].key == recs[i].key && recs[j].win == recs[i].win && recs[j].seq == recs[j - 1].seq + 1) ++j;
        runs.push_back(Run{recs[i].key, segs ? recs[i].win : 0u, recs[i].seq, (uint32_t)(j - i), i});
        i = j;
    }
    std::sort(runs.begin(), runs.end(), [](const Run &x, const Run &y) {
        if (x.seg != y.seg) return x.seg < y.seg;
        return x.key != y.key ? x.key < y.key : x.seq0 < y.seq0;
    });
    void *mem = nullptr;
    int rc = alloc_out(nrecs, sizeof(fz_match), &mem);
    if (rc) return rc;
    fz_match *mo = static_cast<fz_match *>(mem);
    uint32_t *so = nullptr;
    if (seg_out) {
        void *smem_ = nullptr;
        rc = alloc_out(nrecs, sizeof(uint32_t), &smem_);
        if (rc) { release_out(mem); return rc; }
        so = static_cast<uint32_t *>(smem_);
    }
    size_t o = 0;
    for (const Run &run : runs) {
        uint64_t sa = 0;
        if (geom.seg_stride) {                                 // start of segment run.seg (fz_segment)
            const uint64_t core = geom.seg_org + (uint64_t)run.seg * geom.seg_stride;
            sa = core - geom.seg_org >= geom.seg_pre ? core - geom.seg_pre : geom.seg_org;
        }
        for (size_t i = run.first; i < run.first + run.len; ++i, ++o) {
            const FzOutRow row = fz_gen_row(run.key, L, k, sa, recs[i].se, recs[i].dist);
            mo[o].start = row.start; mo[o].end = row.end; mo[o].dist = row.dist; mo[o].block = row.block;
            if (so) so[o] = run.seg;
        }
    }
    if (seg_out) *seg_out = so;
    *out = mo;
    *n = nrecs;
    ctx->stats.raw_matches = nrecs;
    return FZ_OK;
}

}  // namespace

// ---- RCCL without PyTorch ------------------------------------------------
namespace {

int comm_setup_dev(DevState &d) {
    HIP_TRY(hipSetDevice(d.device));
    if (!d.comm_stream) HIP_TRY(hipStreamCreateWithFlags(&d.comm_stream, hipStreamNonBlocking));
    for (ResultSlot &s : d.slots) if (!s.ev_snap) HIP_TRY(hipEventCreateWithFlags(&s.ev_snap, hipEventDisableTiming));
    if (!d.ev_done) HIP_TRY(hipEventCreateWithFlags(&d.ev_done, hipEventDisableTiming));
    return ensure_send(d, d.rec_cap);
}

void comm_teardown(fz_ctx *ctx) {
    if (ctx->comm_broken) {
        // a collective never completed: waiting for its stream or freeing what it may still write would hang as well —
        // the communicator, its streams and buffers are left behind (the process is about to report the failure)
        for (DevState &d : ctx->devs) {
            d.comm = nullptr; d.comm_stream = nullptr; d.d_recv = nullptr; d.h_recv = nullptr; d.recv_bytes = 0; d.send_cap = 0;
            for (ResultSlot &s : d.slots) { s.d_send = nullptr; s.ev_snap = nullptr; s.snap_taken = false; }
            d.ev_done = nullptr; d.comm_rank = -1;
        }
        ctx->comm_world = 0; ctx->snapshot = false; ctx->comm_broken = false;
        return;
    }
    for (DevState &d : ctx->devs) {
        (void)hipSetDevice(d.device);
        if (d.comm_stream) (void)hipStreamSynchronize(d.comm_stream);
        if (d.comm) { if (rccl_api()->ok) (void)rccl_api()->CommDestroy(d.comm); d.comm = nullptr; }
        for (ResultSlot &s : d.slots) {
            if (s.d_send) { (void)hipFree(s.d_send); s.d_send = nullptr; }
            if (s.ev_snap) { (void)hipEventDestroy(s.ev_snap); s.ev_snap = nullptr; }
            s.snap_taken = false;
        }
        d.send_cap = 0;
        if (d.d_recv) { (void)hipFree(d.d_recv); d.d_recv = nullptr; }
        if (d.h_recv) { (void)hipHostFree(d.h_recv); d.h_recv = nullptr; }
        d.recv_bytes = 0;
        if (d.ev_done) { (void)hipEventDestroy(d.ev_done); d.ev_done = nullptr; }
        if (d.comm_stream) { (void)hipStreamDestroy(d.comm_stream); d.comm_stream = nullptr; }
        d.comm_rank = -1;
    }
    ctx->comm_world = 0;
    ctx->snapshot = false;
}

int comm_busy(fz_ctx *ctx) {
    if (!ctx) return fail(FZ_EINVAL, "null argument");
    if (ctx->npend || ctx->stream_inflight) return fail(FZ_EINVAL, "a search of this context is in flight");
    return FZ_OK;
}

// One-process-per-GPU jobs: is this context one rank of several (its own results are only a part of the answer)?
bool comm_multi_process(const fz_ctx *ctx) { return ctx->snapshot && ctx->comm_world > 0 && ctx->devs.size() == 1; }

// nbytes from every rank of a one-process-per-GPU communicator, rank order, through device buffers (blocking).
int comm_allgather_fixed(fz_ctx *ctx, const void *send, uint64_t nbytes, void *recv) {
    if (ctx->comm_broken) return fail(FZ_ETIMEOUT, "the communicator was abandoned after a collective ran into its deadline");
    DevState &d = ctx->devs[0];
    HIP_TRY(hipSetDevice(d.device));
    const uint64_t world = (uint64_t)ctx->comm_world;
    uint8_t *tmp = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&tmp), (world + 1) * nbytes));
    auto body = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(tmp, send, nbytes, hipMemcpyHostToDevice, d.comm_stream));
        NCCL_TRY(rccl_api()->AllGather(tmp, tmp + nbytes, nbytes, ncclChar, d.comm, d.comm_stream));
        HIP_TRY(hipMemcpyAsync(recv, tmp + nbytes, world * nbytes, hipMemcpyDeviceToHost, d.comm_stream));
        return comm_wait(d.comm_stream, "an all-gather over the job's ranks");
    };
    int rc = body();
    if (rc == FZ_ETIMEOUT) ctx->comm_broken = true;        // (and the buffer stays: the stream may still write to it)
    else (void)hipFree(tmp);
    return rc;
}

// The exchange step of the searches whose results reach the host before they are exchanged (exact search: hit
// indices; generic search: automaton records / folded pairs; the linear-programming routes): every rank contributes
// `bytes` bytes of `elem`-byte items, `all` receives the ranks' contributions back to back in rank order.  Two
// all-gathers (sizes, then the payload padded to the largest contribution).  The callers order what they get by keys
// that are global (hit index, block), so the rank order itself carries no meaning.
int comm_gather_host(fz_ctx *ctx, const void *data, uint64_t bytes, std::vector<uint8_t> &all) {
    const auto t_start = std::chrono::steady_clock::now();
    const uint64_t world = (uint64_t)ctx->comm_world;
    std::vector<uint64_t> sizes(world, 0);
    int rc = comm_allgather_fixed(ctx, &bytes, sizeof bytes, sizes.data());
    if (rc) return rc;
    uint64_t top = 0, total = 0;
    for (uint64_t v : sizes) { top = std::max(top, v); total += v; }
    all.clear();
    if (top == 0) return FZ_OK;
    const uint64_t cap = (top + 255) / 256 * 256;
    std::vector<uint8_t> mine(cap, 0), got(world * cap);
    if (bytes) memcpy(mine.data(), data, bytes);
    rc = comm_allgather_fixed(ctx, mine.data(), cap, got.data());
    if (rc) return rc;
    all.resize(total);
    uint64_t o = 0;
    for (uint64_t r = 0; r < world; ++r) {
        if (sizes[r]) memcpy(all.data() + o, got.data() + r * cap, sizes[r]);
        o += sizes[r];
    }
    ctx->last_gather_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    return FZ_OK;
}

// has_near_match_* of a one-process-per-GPU job: true on every rank if any rank found something
int comm_or(fz_ctx *ctx, bool &flag) {
    uint64_t mine = flag ? 1 : 0;
    std::vector<uint64_t> all((size_t)ctx->comm_world, 0);
    int rc = comm_allgather_fixed(ctx, &mine, sizeof mine, all.data());
    if (rc) return rc;
    for (uint64_t v : all) flag = flag || v != 0;
    return FZ_OK;
}

// seq->rank_lo: the first index every rank owns of this sequence.  A multi-device context knows them; the ranks of a
// one-process-per-GPU job exchange them on the sequence's first collective search (every rank is in that search).
int comm_rank_lows(fz_ctx *ctx, fz_seq *seq) {
    const size_t world = (size_t)ctx->comm_world;
    if (seq->rank_lo.size() == world) return FZ_OK;
    seq->rank_lo.assign(world, ~0ull);
    if (ctx->devs.size() == world && world > 1) {
        for (const Shard &sh : seq->shards)
            if (sh.geom.own_hi > sh.geom.own_lo) seq->rank_lo[(size_t)ctx->devs[sh.dev].comm_rank] = sh.geom.own_lo;
        return FZ_OK;
    }
    uint64_t mine = ~0ull;
    for (const Shard &sh : seq->shards) if (sh.geom.own_hi > sh.geom.own_lo) mine = std::min(mine, sh.geom.own_lo);
    int rc = comm_allgather_fixed(ctx, &mine, sizeof mine, seq->rank_lo.data());
    if (rc) seq->rank_lo.clear();
    return rc;
}

}  // namespace

extern "C" {

int fz_comm_unique_id(void *id, uint64_t id_bytes) {
    static_assert(FZ_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");
    if (!id || id_bytes < FZ_COMM_ID_BYTES) return fail(FZ_EINVAL, "the id buffer must hold %d bytes", FZ_COMM_ID_BYTES);
    RCCL_NEED();
    ncclUniqueId u;
    NCCL_TRY(rccl_api()->GetUniqueId(&u));
    memcpy(id, u.internal, FZ_COMM_ID_BYTES);
    return FZ_OK;
}

int fz_comm_init_rank(fz_ctx *ctx, const void *id, int world, int rank) {
    int rc = comm_busy(ctx);
    if (rc) return rc;
    if (!id || world < 1 || rank < 0 || rank >= world) return fail(FZ_EINVAL, "bad communicator arguments");
    if (ctx->devs.size() != 1) return fail(FZ_EINVAL, "fz_comm_init_rank needs a single-device context (one process per GPU); use fz_comm_init_all");
    if (ctx->comm_world) return fail(FZ_EINVAL, "the context already joined a communicator");
    RCCL_NEED();
    DevState &d = ctx->devs[0];
    rc = comm_setup_dev(d);
    if (rc) return rc;
    ncclUniqueId u;
    memcpy(u.internal, id, FZ_COMM_ID_BYTES);
    NCCL_TRY(rccl_api()->CommInitRank(&d.comm, world, u, rank));
    d.comm_rank = rank;
    ctx->comm_world = world;
    ctx->snapshot = true;
    return FZ_OK;
}

int fz_comm_init_all(fz_ctx *ctx) {
    int rc = comm_busy(ctx);
    if (rc) return rc;
    if (ctx->comm_world) return fail(FZ_EINVAL, "the context already joined a communicator");
    RCCL_NEED();
    const int nd = (int)ctx->devs.size();
    std::vector<int> ids(nd);
    for (int i = 0; i < nd; ++i) {
        ids[i] = ctx->devs[i].device;
        // RCCL refuses two ranks on one GPU; the test suite's stand-in library (tests/mock_rccl.cpp, loaded through
        // FZ_RCCL_LIB) does not, which is how the N-rank code runs where there is only one device
        for (int j = 0; j < i && !rccl_api()->stand_in; ++j)
            if (ids[j] == ids[i]) return fail(FZ_EUNSUPPORTED, "device %d appears twice in the context: RCCL needs one rank per GPU", ids[i]);
    }
    for (DevState &d : ctx->devs) { rc = comm_setup_dev(d); if (rc) return rc; }
    std::vector<ncclComm_t> comms(nd, nullptr);
    NCCL_TRY(rccl_api()->CommInitAll(comms.data(), nd, ids.data()));
    for (int i = 0; i < nd; ++i) { ctx->devs[i].comm = comms[i]; ctx->devs[i].comm_rank = i; }
    ctx->comm_world = nd;
    ctx->snapshot = true;
    return FZ_OK;
}

int fz_comm_info(fz_ctx *ctx, int *world, int *rank, int *collective) {
    if (!ctx) return fail(FZ_EINVAL, "null argument");
    if (world) *world = ctx->comm_world;
    if (rank) *rank = ctx->comm_world ? ctx->devs[0].comm_rank : -1;
    if (collective) *collective = ctx->snapshot ? 1 : 0;
    return FZ_OK;
}

int fz_comm_set_collective(fz_ctx *ctx, int on) {
    int rc = comm_busy(ctx);
    if (rc) return rc;
    if (!ctx->comm_world) return fail(FZ_EINVAL, "the context has not joined a communicator");
    ctx->snapshot = on != 0;
    return FZ_OK;
}

void fz_comm_destroy(fz_ctx *ctx) {
    if (ctx) comm_teardown(ctx);
}

// host buffers: nbytes from every rank, rank order (load-time exchanges: halos, the job's clock)
int fz_comm_allgather(fz_ctx *ctx, const void *send, uint64_t nbytes, void *recv) {
    int rc = comm_busy(ctx);
    if (rc) return rc;
    if (!ctx->comm_world) return fail(FZ_EINVAL, "the context has not joined a communicator");
    if (ctx->devs.size() != 1) return fail(FZ_EINVAL, "fz_comm_allgather is for one-process-per-GPU jobs (a multi-device context holds every rank's data itself)");
    if (!nbytes) return FZ_OK;
    if (!send || !recv) return fail(FZ_EINVAL, "null argument");
    return comm_allgather_fixed(ctx, send, nbytes, recv);
}

// max over the ranks of one double per rank (the job's step time); doubles as a barrier
int fz_comm_max_f64(fz_ctx *ctx, double *value) {
    int rc = comm_busy(ctx);
    if (rc) return rc;
    if (!ctx->comm_world || !value) return fail(FZ_EINVAL, "no communicator / null argument");
    if (ctx->devs.size() != 1) return FZ_OK;               // one process holds every rank: nothing to reduce
    if (ctx->comm_broken) return fail(FZ_ETIMEOUT, "the communicator was abandoned after a collective ran into its deadline");
    DevState &d = ctx->devs[0];
    HIP_TRY(hipSetDevice(d.device));
    double *tmp = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&tmp), sizeof(double)));
    auto body = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(tmp, value, sizeof(double), hipMemcpyHostToDevice, d.comm_stream));
        NCCL_TRY(rccl_api()->AllReduce(tmp, tmp, 1, ncclDouble, ncclMax, d.comm, d.comm_stream));
        HIP_TRY(hipMemcpyAsync(value, tmp, sizeof(double), hipMemcpyDeviceToHost, d.comm_stream));
        return comm_wait(d.comm_stream, "an all-reduce over the job's ranks");
    };
    rc = body();
    if (rc == FZ_ETIMEOUT) ctx->comm_broken = true;
    else (void)hipFree(tmp);
    return rc;
}

int fz_comm_barrier(fz_ctx *ctx) {
    if (ctx) for (DevState &d : ctx->devs) { (void)hipSetDevice(d.device); (void)hipStreamSynchronize(d.stream); (void)hipStreamSynchronize(d.stream_alt); }
    double one = 1.0;
    return fz_comm_max_f64(ctx, &one);
}

// Test hook: read the FZ_* switches from the environment again (they are read once, on first use; a test that changes one
// inside a running process calls this — no search may be in flight anywhere in the process).
void fz_debug_reload_switches(void) { switches_storage() = read_switches(); }

int fz_comm_backend(void) { return !rccl_api()->ok ? 0 : rccl_api()->stand_in ? 2 : 1; }

int fz_comm_gather_ms(fz_ctx *ctx, double *ms) {
    if (!ctx || !ms) return fail(FZ_EINVAL, "null argument");
    *ms = ctx->last_gather_ms;
    return FZ_OK;
}

int fz_debug_scan_regions(uint64_t ntiles, uint64_t grid, uint32_t n_cus, int steps, double fmin, int wg_per_cu, uint32_t *n_regions,
                          uint64_t *table) {
    if (!n_regions || !table) return fail(FZ_EINVAL, "null argument");
    static FzScanArgs fa;                                   // (1.7 KB: not on the stack of a ctypes call for nothing)
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    plan_scan_regions(fa, ntiles, grid, n_cus, steps, fmin, wg_per_cu);
    *n_regions = fa.nreg;
    for (uint32_t r = 0; r < fa.nreg; ++r) {
        table[4 * r] = fa.reg_wg0[r]; table[4 * r + 1] = fa.reg_nwg[r]; table[4 * r + 2] = fa.reg_tile0[r]; table[4 * r + 3] = fa.reg_end[r];
    }
    return FZ_OK;
}

int fz_debug_scan_plan(const uint8_t *p, uint32_t m, uint32_t k, uint64_t buf_len, uint32_t n_cus, int shares_chip, uint32_t *grid,
                       uint32_t *form, int *overlapped, uint32_t *n_regions, uint64_t *table) {
    if (!p || !grid || !form || !overlapped || !n_regions || !table || m == 0 || m / (k + 1) == 0 || n_cus == 0)
        return fail(FZ_EINVAL, "bad argument");
    Search q;                                               // what lev_plan makes of the search, without a context
    q.mode = FZ_MODE_LEV; q.m = m; q.k = k; q.p = p;
    q.plan.L = m / (k + 1);
    for (uint32_t s = 0; s + q.plan.L <= m; s += q.plan.L) q.plan.s.push_back(s);
    FzGeom geom{};
    geom.buf_len = buf_len;
    static FzScanArgs fa;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    memset(&fa, 0, sizeof fa);
    const ScanPlan sp = plan_scan(q, geom, n_cus, true, shares_chip != 0, fa);
    *grid = sp.grid;
    *form = sp.form;
    *overlapped = sp.overlapped ? 1 : 0;
    *n_regions = fa.nreg;
    for (uint32_t r = 0; r < fa.nreg; ++r) {
        table[4 * r] = fa.reg_wg0[r]; table[4 * r + 1] = fa.reg_nwg[r]; table[4 * r + 2] = fa.reg_tile0[r]; table[4 * r + 3] = fa.reg_end[r];
    }
    return FZ_OK;
}

int fz_debug_scan_walk(uint64_t ntiles, uint32_t grid, uint32_t n_regions, const uint64_t *table, uint32_t wg, uint32_t iter,
                       int reversed, uint64_t *tile) {
    if (!tile || (n_regions && !table) || n_regions > FZ_MAX_REGIONS || grid == 0 || wg >= grid) return fail(FZ_EINVAL, "bad argument");
    uint32_t wg0[FZ_MAX_REGIONS] = {0}, nwg[FZ_MAX_REGIONS] = {0};
    uint64_t tile0[FZ_MAX_REGIONS] = {0}, end[FZ_MAX_REGIONS] = {0};
    for (uint32_t r = 0; r < n_regions; ++r) {
        wg0[r] = (uint32_t)table[4 * r]; nwg[r] = (uint32_t)table[4 * r + 1]; tile0[r] = table[4 * r + 2]; end[r] = table[4 * r + 3];
    }
    *tile = fz_walk_tile(fz_scan_walk(n_regions, wg0, nwg, tile0, end, grid, ntiles, wg, reversed != 0), iter);
    return FZ_OK;
}

int fz_debug_scan_direction(fz_ctx *ctx, fz_seq *seq, int *next_reversed, uint64_t *reversed_launches) {
    if (!ctx || !next_reversed || !reversed_launches) return fail(FZ_EINVAL, "null argument");
    const bool at_end = seq && !seq->shards.empty() && seq->shards[0].scan_at_end;       // (every shard has its own bit: the first one's)
    *next_reversed = (ctx->scan_dir == 2 || (ctx->scan_dir == 0 && at_end)) ? 1 : 0;
    *reversed_launches = ctx->rev_launches.load(std::memory_order_relaxed);
    return FZ_OK;
}

int fz_debug_scan_instance(uint32_t mode, const uint8_t *p, uint32_t m, uint32_t k, uint64_t buf_len, uint32_t n_cus,
                           uint32_t *n_launches, uint32_t *lean_mask, uint32_t *form) {
    if (!p || !n_launches || !lean_mask || !form || m == 0 || m / (k + 1) == 0 || n_cus == 0 || (mode != FZ_MODE_LEV && mode != FZ_MODE_SUBS))
        return fail(FZ_EINVAL, "bad argument");
    Search q;                                               // what lev_plan / subs_plan make of the search, without a context
    q.mode = mode; q.m = m; q.k = k; q.p = p;
    q.plan.L = m / (k + 1);
    for (uint32_t s = 0; s + q.plan.L <= m; s += q.plan.L) q.plan.s.push_back(s);
    if (q.plan.s.size() > FZ_MAX_BLOCKS) return fail(FZ_EUNSUPPORTED, "more than %u n-gram blocks", FZ_MAX_BLOCKS);
    FzGeom geom{};
    geom.buf_len = buf_len;
    static FzScanArgs fa;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    memset(&fa, 0, sizeof fa);
    const ScanPlan sp = plan_scan(q, geom, n_cus, true, false, fa);
    const HashGeom hgeom(q.plan.L);
    fa.d2 = hgeom.nwin == 2 ? std::min<uint32_t>(q.plan.L, 8) - 4 : 0;
    fa.mask1 = hgeom.mask1;
    uint32_t nl = 0, mask = 0;
    for (uint32_t g0 = 0; g0 < q.plan.s.size(); ++nl) {
        const uint32_t nblk = fill_launch_blocks(fa, q, g0, hgeom);
        if (nblk == 0) return fail(FZ_EDEVICE, "internal: a launch without blocks");
        if (nl < 32 && scan_is_lean(q.mode, q.k, fa, sp.wfg, false, false)) mask |= 1u << nl;
        g0 += nblk;
    }
    *n_launches = nl;
    *lean_mask = mask;
    *form = sp.form;
    return FZ_OK;
}

int fz_debug_gather_merge(const void *blocks, uint32_t world, uint64_t cap, const uint64_t *own_lo, uint32_t L, fz_match **out,
                          uint64_t *n_out, uint64_t *need_cap) {
    if (!blocks || !out || !n_out || !need_cap || world == 0) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *n_out = 0; *need_cap = 0;
    std::vector<FzRec> recs;
    std::vector<size_t> seg_ends;
    std::vector<uint32_t> seg_order;
    uint64_t top = 0, total = 0;
    parse_gathered(static_cast<const uint8_t *>(blocks), (int)world, kHeaderBytes + cap * sizeof(FzRec), cap, own_lo, recs, seg_ends,
                   seg_order, &top, &total);
    if (top > cap) { *need_cap = (top + top / 4 + 1023) / 1024 * 1024; return FZ_OK; }
    return emit_matches_segments(nullptr, recs.data(), seg_ends, seg_order, L, out, n_out, 0, 0, true);
}

}  // extern "C"

// ---- (f)3: the reference's linear-programming fallbacks for short patterns, on the GPU ---------
namespace {

struct LpRec { int64_t start, end; int32_t dist; uint64_t step; uint64_t w0; uint32_t seq; };

constexpr uint32_t kLpStarts = 256;      // start positions owned by one window (one wave)

// Whole-sequence automaton (generic or Levenshtein), tiled by start position: tile w spawns the
// candidates of starts [w0, w0 + 256) and runs them over [w0, w0 + 256 + m + k) — a candidate lives
// at most m - 1 + k characters, so tiles are independent; only the tile reaching the sequence end
// performs the reference's end-of-sequence flush.
int run_lp(fz_ctx *ctx, fz_seq *seq, const Search &q, uint32_t lp_kind, std::vector<LpRec> &out) {
    // tile-relative start / end travel in 16 bits each: a tile's window is m + 2k + kLpStarts bytes
    if ((uint64_t)q.m + 2ull * q.k + kLpStarts > 65535ull)
        return fail(FZ_EUNSUPPORTED, "linear-programming route: len(subsequence) + 2 * max_l_dist + %u = %llu exceeds 65535 (16-bit window coordinates)",
                    kLpStarts, (unsigned long long)q.m + 2ull * q.k + kLpStarts);
    memset(&ctx->stats, 0, sizeof ctx->stats); ctx->tref.clear();
    ctx->stats.n_devices = (uint32_t)ctx->devs.size();
    uint32_t cand_cap = 1024;
    for (int attempt = 0; attempt < 8; ++attempt) {
        out.clear();
        bool rerun = false;
        const uint32_t mpad = (q.m + 15u) & ~15u, wpad = (q.m + 2 * q.k + kLpStarts + 15u) & ~15u;
        for (const Shard &sh : seq->shards) {
            DevState &d = ctx->devs[sh.dev];
            HIP_TRY(hipSetDevice(d.device));
            size_t lds = 0;
            uint64_t scratch = 0;
            int rc_lists = cand_lists(d, cand_cap, mpad + wpad + FZ_GEN_MCAP * 8, lds, scratch);
            if (rc_lists) return rc_lists;
            unsigned long long *counters = reinterpret_cast<unsigned long long *>(d.d_out);
            FzGenRec *recs = reinterpret_cast<FzGenRec *>(d.d_out + kHeaderBytes);
            HIP_TRY(hipMemsetAsync(d.d_out, 0, kHeaderBytes, d.stream));
            d.header_zeroed = false;
            HIP_TRY(hipEventRecord(d.cur().ev[0], d.stream));
            FzScanArgs fa;
            memset(&fa, 0, sizeof fa);
            fa.geom = sh.geom;
            fa.mode = q.mode; fa.m = q.m; fa.k = q.k; fa.L = 0;
            fa.max_subs = q.max_subs; fa.max_ins = q.max_ins; fa.max_dels = q.max_dels;
            fa.cand_cap = cand_cap;
            fa.cand_scratch = scratch;
            fa.lp_kind = lp_kind;
            fa.lp_starts = kLpStarts;
            fa.rec_cap = d.rec_cap;
            if (q.m <= FZ_MAX_M) memcpy(fa.pat, q.p, q.m);
            { int rcp = stage_pattern(d, fa, q.p, q.m); if (rcp) return rcp; }
            const uint64_t own = sh.geom.own_hi - sh.geom.own_lo;
            const uint64_t nwin = (own + kLpStarts - 1) / kLpStarts;
            if (lds > 64 * 1024)
                HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(lp_kernel(lp_kind, scratch != 0)),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            if (nwin) {
                const unsigned grid = (unsigned)std::min<uint64_t>(nwin, scratch ? kCandScratchGrid : (uint64_t)d.n_cus * 64);
                hipLaunchKernelGGL(lp_kernel(lp_kind, scratch != 0), dim3(grid), dim3(64), lds, d.stream, sh.d_buf, fa, d.d_hits,
                                   nwin, recs, counters);
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(hipEventRecord(d.cur().ev[1], d.stream));
            HIP_TRY(hipMemcpyAsync(d.cur().h_stage, d.d_out, kHeaderBytes + kFirstCopyRecs * sizeof(FzRec),
                                   hipMemcpyDeviceToHost, d.stream));
            HIP_TRY(hipEventRecord(d.cur().ev[3], d.stream));
        }
        for (const Shard &sh : seq->shards) {
            DevState &d = ctx->devs[sh.dev];
            HIP_TRY(hipSetDevice(d.device));
            HIP_TRY(hipStreamSynchronize(d.stream));
            const unsigned long long *cnt = reinterpret_cast<const unsigned long long *>(d.cur().h_stage);
            const uint64_t nr = cnt[1], novf = cnt[2];
            if (nr > d.rec_cap) { int rc = ensure_recs(d, nr + nr / 8 + 1024); if (rc) return rc; rerun = true; }
            if (novf) { cand_cap *= 4; rerun = true; }
            if (rerun) continue;
            float f = 0, t = 0;
            HIP_TRY(hipEventElapsedTime(&f, d.cur().ev[0], d.cur().ev[1]));
            HIP_TRY(hipEventElapsedTime(&t, d.cur().ev[0], d.cur().ev[3]));
            ctx->stats.verify_ms = std::max<double>(ctx->stats.verify_ms, f);
            ctx->stats.device_ms = std::max<double>(ctx->stats.device_ms, t);
            ctx->stats.bytes_scanned += sh.geom.buf_len;
            std::vector<FzGenRec> tmp(nr);
            const uint64_t first = std::min<uint64_t>(nr, kFirstCopyRecs);
            if (first) memcpy(tmp.data(), d.cur().h_stage + kHeaderBytes, first * sizeof(FzGenRec));
            if (nr > first)
                HIP_TRY(hipMemcpy(tmp.data() + first, d.d_out + kHeaderBytes + first * sizeof(FzGenRec),
                                  (nr - first) * sizeof(FzGenRec), hipMemcpyDeviceToHost));
            for (const FzGenRec &r : tmp) {
                LpRec o;
                o.w0 = sh.geom.own_lo + (uint64_t)r.win * kLpStarts;
                o.start = (int64_t)(o.w0 + (r.se & 0xffffu));
                o.end = (int64_t)(o.w0 + (r.se >> 16));
                o.dist = (int32_t)r.dist;
                o.step = r.key;
                o.seq = r.seq;
                out.push_back(o);
            }
        }
        if (!rerun) { ctx->stats.raw_matches = out.size(); return FZ_OK; }
    }
    return fail(FZ_EUNSUPPORTED, "automaton candidate lists / result buffers kept overflowing");
}

// one-process-per-GPU jobs: the ranks' records back to back (emit_lp orders them by step / tile / list position,
// all of which are global)
int lp_exchange(fz_ctx *ctx, std::vector<LpRec> &recs) {
    if (!comm_multi_process(ctx)) return FZ_OK;
    std::vector<uint8_t> all;
    int rc = comm_gather_host(ctx, recs.data(), recs.size() * sizeof(LpRec), all);
    if (rc) return rc;
    recs.resize(all.size() / sizeof(LpRec));
    if (!all.empty()) memcpy(static_cast<void *>(recs.data()), all.data(), all.size());
    ctx->stats.raw_matches = recs.size();
    return FZ_OK;
}

int emit_lp(std::vector<LpRec> &recs, bool newest_first, fz_match **out, uint64_t *n) {
    // reference emission order: by sequence step; within a step by candidate-list order, i.e. by
    // start ascending (generic: fresh candidates are appended) or descending (Levenshtein: the fresh
    // candidate goes first); within one tile the kernel already kept list order (seq).
    std::sort(recs.begin(), recs.end(), [newest_first](const LpRec &a, const LpRec &b) {
        if (a.step != b.step) return a.step < b.step;
        if (a.w0 != b.w0) return newest_first ? a.w0 > b.w0 : a.w0 < b.w0;
        return a.seq < b.seq;
    });
    void *mem = nullptr;
    int rc = alloc_out(recs.size(), sizeof(fz_match), &mem);
    if (rc) return rc;
    fz_match *mo = static_cast<fz_match *>(mem);
    for (size_t i = 0; i < recs.size(); ++i) {
        mo[i].start = recs[i].start; mo[i].end = recs[i].end; mo[i].dist = recs[i].dist; mo[i].block = -1;
    }
    *out = mo;
    *n = recs.size();
    return FZ_OK;
}

}  // namespace

extern "C" int fz_lev_lp(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, fz_match **out, uint64_t *n) {
    if (!out || !n) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *n = 0;
    int rc = validate(ctx, seq, p, m);
    if (rc) return rc;
    if (k >= m) {                                              // levenshtein.py:62-65: data independent
        const uint64_t cnt = seq->n + 1;
        void *mem = nullptr;
        rc = alloc_out(cnt, sizeof(fz_match), &mem);
        if (rc) return rc;
        fz_match *mo = static_cast<fz_match *>(mem);
        for (uint64_t i = 0; i < cnt; ++i) { mo[i].start = mo[i].end = (int64_t)i; mo[i].dist = (int32_t)m; mo[i].block = -1; }
        *out = mo; *n = cnt;
        return FZ_OK;
    }
    if (k > FZ_MAX_K) return fail(FZ_EUNSUPPORTED, "max_l_dist above %d is not supported", FZ_MAX_K);
    rc = check_halo(seq, (uint64_t)m + k);
    if (rc) return rc;
    Search q;
    q.mode = FZ_MODE_LEV; q.m = m; q.k = k; q.p = p;
    std::vector<LpRec> recs;
    rc = run_lp(ctx, seq, q, FZ_LP_LEV_SEQ, recs);
    if (rc == FZ_OK) rc = lp_exchange(ctx, recs);
    if (rc) return rc;
    return emit_lp(recs, /*newest_first=*/true, out, n);
}

extern "C" int fz_generic_lp(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t max_subs, uint32_t max_ins,
                             uint32_t max_dels, uint32_t max_l, fz_match **out, uint64_t *n) {
    if (!out || !n) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *n = 0;
    int rc = validate(ctx, seq, p, m);
    if (rc) return rc;
    if (max_l > FZ_MAX_K) return fail(FZ_EUNSUPPORTED, "max_l_dist above %d is not supported", FZ_MAX_K);
    rc = check_halo(seq, (uint64_t)m + max_l);
    if (rc) return rc;
    Search q;
    q.mode = FZ_MODE_GENERIC; q.m = m; q.k = max_l; q.p = p;
    q.max_subs = std::min(max_subs, 255u); q.max_ins = std::min(max_ins, 255u); q.max_dels = std::min(max_dels, 255u);
    std::vector<LpRec> recs;
    rc = run_lp(ctx, seq, q, FZ_LP_GENERIC_SEQ, recs);
    if (rc == FZ_OK) rc = lp_exchange(ctx, recs);
    if (rc) return rc;
    return emit_lp(recs, /*newest_first=*/false, out, n);
}

static int subs_lp_impl(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, fz_match **out, uint64_t *n, int *found);

extern "C" int fz_subs_lp(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, fz_match **out, uint64_t *n) {
    if (!out || !n) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *n = 0;
    return subs_lp_impl(ctx, seq, p, m, k, out, n, nullptr);
}

extern "C" int fz_subs_lp_any(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, int *found) {
    if (!found) return fail(FZ_EINVAL, "null argument");
    *found = 0;
    return subs_lp_impl(ctx, seq, p, m, k, nullptr, nullptr, found);
}

static int subs_lp_impl(fz_ctx *ctx, fz_seq *seq, const uint8_t *p, uint32_t m, uint32_t k, fz_match **out, uint64_t *n, int *found) {
    int rc = validate(ctx, seq, p, m);
    if (rc) return rc;
    rc = check_halo(seq, m);
    if (rc) return rc;
    memset(&ctx->stats, 0, sizeof ctx->stats); ctx->tref.clear();
    ctx->stats.n_devices = (uint32_t)ctx->devs.size();
    std::vector<FzRec> recs;
    for (int attempt = 0; attempt < 4; ++attempt) {
        recs.clear();
        bool rerun = false;
        for (const Shard &sh : seq->shards) {
            DevState &d = ctx->devs[sh.dev];
            HIP_TRY(hipSetDevice(d.device));
            unsigned long long *counters = reinterpret_cast<unsigned long long *>(d.d_out);
            FzRec *drecs = reinterpret_cast<FzRec *>(d.d_out + kHeaderBytes);
            HIP_TRY(hipMemsetAsync(d.d_out, 0, kHeaderBytes, d.stream));
            d.header_zeroed = false;
            FzScanArgs fa;
            memset(&fa, 0, sizeof fa);
            fa.geom = sh.geom; fa.mode = FZ_MODE_SUBS; fa.m = m; fa.k = k; fa.rec_cap = d.rec_cap;
            fa.flags = found ? FZ_FLAG_ANY : 0u;
            if (m <= FZ_MAX_M) memcpy(fa.pat, p, m);
            rc = stage_pattern(d, fa, p, m);
            if (rc) return rc;
            const uint64_t own = sh.geom.own_hi - sh.geom.own_lo;
            const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((own + 255) / 256, (uint64_t)d.n_cus * 16));
            hipLaunchKernelGGL(fz_hamming_kernel, dim3(grid), dim3(256), 0, d.stream, sh.d_buf, fa, drecs, counters);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(d.cur().h_stage, d.d_out, kHeaderBytes + kFirstCopyRecs * sizeof(FzRec),
                                   hipMemcpyDeviceToHost, d.stream));
        }
        for (const Shard &sh : seq->shards) {
            DevState &d = ctx->devs[sh.dev];
            HIP_TRY(hipSetDevice(d.device));
            HIP_TRY(hipStreamSynchronize(d.stream));
            const unsigned long long *cnt = reinterpret_cast<const unsigned long long *>(d.cur().h_stage);
            const uint64_t nr = cnt[1];
            if (found) { if (nr) *found = 1; continue; }
            if (nr > d.rec_cap) { rc = ensure_recs(d, nr + nr / 8 + 1024); if (rc) return rc; rerun = true; continue; }
            const size_t base = recs.size();
            recs.resize(base + nr);
            const uint64_t first = std::min<uint64_t>(nr, kFirstCopyRecs);
            if (first) memcpy(recs.data() + base, d.cur().h_stage + kHeaderBytes, first * sizeof(FzRec));
            if (nr > first)
                HIP_TRY(hipMemcpy(recs.data() + base + first, d.d_out + kHeaderBytes + first * sizeof(FzRec),
                                  (nr - first) * sizeof(FzRec), hipMemcpyDeviceToHost));
            ctx->stats.bytes_scanned += sh.geom.buf_len;
        }
        if (!rerun) break;
        if (attempt == 3) return fail(FZ_EDEVICE, "result buffers kept overflowing");
    }
    if (found) {
        bool any = *found != 0;
        if (comm_multi_process(ctx)) { rc = comm_or(ctx, any); if (rc) return rc; }
        *found = any ? 1 : 0;
        return FZ_OK;
    }
    if (comm_multi_process(ctx)) {
        std::vector<uint8_t> all;
        rc = comm_gather_host(ctx, recs.data(), recs.size() * sizeof(FzRec), all);
        if (rc) return rc;
        recs.resize(all.size() / sizeof(FzRec));
        if (!all.empty()) memcpy(static_cast<void *>(recs.data()), all.data(), all.size());
    }
    sort_recs(recs);
    void *mem = nullptr;
    rc = alloc_out(recs.size(), sizeof(fz_match), &mem);
    if (rc) return rc;
    fz_match *mo = static_cast<fz_match *>(mem);
    for (size_t i = 0; i < recs.size(); ++i) {
        mo[i].start = (int64_t)recs[i].key; mo[i].end = (int64_t)recs[i].key + m; mo[i].dist = (int32_t)recs[i].dist; mo[i].block = -1;
    }
    *out = mo; *n = recs.size();
    ctx->stats.raw_matches = recs.size();
    return FZ_OK;
}

// ---- (f)2 / a12: find_near_matches_in_file as a pipeline -------------------------------------------
// The reference reads a file in chunks and searches every chunk as an independent sequence
// (__init__.py:129-200).  Here the file crosses PCIe in large batches (many chunks each) from pinned,
// double-buffered staging memory; the chunks of a batch are SEGMENTS of one resident buffer with their
// own clamps (FzGeom), searched by one launch, while the host already fills the next staging buffer.
struct fz_stream {
    fz_ctx *ctx = nullptr;
    uint32_t mode = 0, m = 0, k = 0, max_subs = 0, max_ins = 0, max_dels = 0;
    std::vector<uint8_t> pat;
    uint64_t S = 0;                      // segment stride
    uint32_t pre = 0, post = 0;          // segment j = [j*S - pre, (j+1)*S + post) clipped to the file
    uint64_t cap = 0;                    // bytes a staging buffer holds
    uint64_t cap_alloc = 0;              // bytes the staging allocations really have (reused buffers may be larger)
    uint8_t *h_buf[2] = {nullptr, nullptr};   // pinned staging
    int cur = 0;                         // staging buffer being filled
    uint64_t stage_off = 0;              // file offset of h_buf[cur][0]
    uint64_t stage_len = 0;              // valid bytes in h_buf[cur]
    uint64_t next_seg = 0;               // first segment not launched yet
    bool eof = false;
    fz_seq *seq = nullptr;               // one transient shard over the device batch buffer
    bool inflight = false;
    uint64_t fl_j0 = 0, fl_j1 = 0;       // segments of the batch in flight
    Search q;
    std::vector<fz_match> out;
    std::vector<uint32_t> out_seg;
    uint64_t bytes_total = 0;
    double t_fill = 0, t_collect = 0, t_launch = 0, t_carry = 0;   // FZ_STREAM_TRACE=1: where the host's time went (ms)
};

namespace {

uint64_t stream_segments_at_eof(const fz_stream *st, uint64_t F) {
    if (F == 0) return 0;
    if (F <= st->post) return 1;
    return (F - st->post - 1) / st->S + 1;                 // segment j >= 1 exists iff j*S + post < F
}

// segment that owns the window [i0, i0 + m) of an exact / substitutions-only match: such windows fit
// exactly one chunk (the overlap is m - 1 items)
uint64_t stream_window_segment(const fz_stream *st, uint64_t i0) {
    return st->post ? i0 / st->S : (i0 + st->m - 1) / st->S;
}

int stream_build_search(fz_stream *st) {
    Search &q = st->q;
    q = Search();
    q.mode = st->mode; q.m = st->m; q.k = st->k; q.p = st->pat.data();
    q.max_subs = st->max_subs; q.max_ins = st->max_ins; q.max_dels = st->max_dels;
    if (st->mode == FZ_MODE_EXACT) {
        q.plan.L = st->m;
        q.plan.s = {0};
        return FZ_OK;
    }
    const uint32_t L = st->m / (st->k + 1);
    if (L == 0) return fail(FZ_EINVAL, "the subsequence length must be greater than the distance limit");
    q.plan.L = L;
    for (uint32_t s = 0; s + L <= st->m; s += L) q.plan.s.push_back(s);
    if (q.plan.s.size() > FZ_MAX_BLOCKS) return fail(FZ_EUNSUPPORTED, "more than %u n-gram blocks", FZ_MAX_BLOCKS);
    return FZ_OK;
}

int stream_collect(fz_stream *st) {
    if (!st->inflight) return FZ_OK;
    fz_ctx *ctx = st->ctx;
    st->inflight = false;
    ctx->stream_inflight = nullptr;
    const uint32_t L = st->q.plan.L;
    fz_match *mo = nullptr;
    uint32_t *so = nullptr;
    uint64_t cnt = 0;
    int rc = FZ_OK;
    if (st->mode == FZ_MODE_GENERIC) {
        std::vector<FzGenRec> recs;
        rc = run_generic(ctx, st->seq, st->q, recs);
        if (rc) return rc;
        rc = emit_generic(ctx, st->seq, recs, L, st->k, &mo, &cnt, &so);
        if (rc) return rc;
    } else {
        std::vector<FzRec> recs;
        std::vector<uint64_t> hits;
        const bool with_verify = st->mode != FZ_MODE_EXACT;
        rc = search_collect(ctx, st->seq, st->q, with_verify, recs, hits);
        if (rc) return rc;
        if (st->mode == FZ_MODE_LEV) {
            const FzRec *r = ctx->view ? ctx->view : recs.data();
            const size_t nr = ctx->view ? (size_t)ctx->view_n : recs.size();
            rc = emit_matches_seg(r, nr, L, &mo, &cnt, &so);
            if (rc) return rc;
        } else {
            // exact / substitutions-only: no clamp depends on the chunk; the chunk of a window follows from
            // its position, and this batch keeps the windows of its own chunks
            std::vector<fz_match> tmp;
            if (st->mode == FZ_MODE_EXACT) {
                std::sort(hits.begin(), hits.end());
                tmp.resize(hits.size());
                for (size_t i = 0; i < hits.size(); ++i) {
                    const int64_t idx = (int64_t)fz_hit_index(hits[i]);
                    tmp[i] = fz_match{idx, idx + (int64_t)st->m, 0, 0};
                }
            } else {
                fz_match *em = nullptr;
                uint64_t en = 0;
                rc = emit_matches(ctx, recs, L, &em, &en);
                if (rc) return rc;
                tmp.assign(em, em + en);
                release_out(em);
            }
            std::vector<std::pair<uint64_t, uint32_t>> order;      // (segment, position in tmp)
            for (size_t i = 0; i < tmp.size(); ++i) {
                const uint64_t j = stream_window_segment(st, (uint64_t)tmp[i].start);
                if (j >= st->fl_j0 && j < st->fl_j1) order.emplace_back(j, (uint32_t)i);
            }
            std::stable_sort(order.begin(), order.end(), [](const std::pair<uint64_t, uint32_t> &x, const std::pair<uint64_t, uint32_t> &y) { return x.first < y.first; });
            for (const auto &o : order) { st->out.push_back(tmp[o.second]); st->out_seg.push_back((uint32_t)o.first); }
            return FZ_OK;
        }
    }
    st->out.insert(st->out.end(), mo, mo + cnt);
    st->out_seg.insert(st->out_seg.end(), so, so + cnt);
    release_out(mo);
    release_out(so);
    return FZ_OK;
}

// Upload the staged bytes the segments [j0, j1) need and launch their search (asynchronous).
int stream_launch(fz_stream *st, uint64_t j0, uint64_t j1, uint64_t data_hi) {
    fz_ctx *ctx = st->ctx;
    // the context's result slots, counters and hit list serve ONE search at a time
    if (ctx->npend || (ctx->stream_inflight && ctx->stream_inflight != st))
        return fail(FZ_EINVAL, "another search or file stream of this context is in flight");
    DevState &d = ctx->devs[0];
    Shard &sh = st->seq->shards[0];
    HIP_TRY(hipSetDevice(d.device));
    const uint64_t len = data_hi - st->stage_off;
    FzGeom g{};
    g.n = data_hi;
    g.buf_off = st->stage_off;
    g.buf_len = len;
    g.own_lo = 0;
    g.own_hi = data_hi;
    const bool segmented = st->mode == FZ_MODE_LEV || st->mode == FZ_MODE_GENERIC;
    if (segmented) {
        g.seg_stride = st->S; g.seg_org = 0; g.seg_pre = st->pre; g.seg_post = st->post;
        g.seg_j0 = j0; g.seg_j1 = j1;
    }
    sh.geom = g;
    st->seq->n = data_hi;
    if (len) HIP_TRY(hipMemcpyAsync(sh.d_buf, st->h_buf[st->cur], len, hipMemcpyHostToDevice, d.stream));
    const uint64_t tiles = (len + FZ_TILE_BYTES - 1) / FZ_TILE_BYTES;
    const uint64_t body = std::max<uint64_t>(1, tiles) * FZ_TILE_BYTES;
    HIP_TRY(hipMemsetAsync(sh.d_buf + len, 0, body + FZ_PAD_BACK - len, d.stream));
    st->fl_j0 = j0;
    st->fl_j1 = j1;
    int rc = ensure_hits(d, std::max<uint64_t>(1u << 20, len / 64));
    if (rc) return rc;
    if (st->mode != FZ_MODE_GENERIC) {
        memset(&ctx->stats, 0, sizeof ctx->stats); ctx->tref.clear();
        ctx->stats.n_devices = 1;
        rc = search_enqueue(ctx, st->seq, st->q, st->mode != FZ_MODE_EXACT, false, /*forward=*/true);   // a batch of file chunks: read once
        if (rc) return rc;
    }
    st->inflight = true;
    ctx->stream_inflight = st;
    return FZ_OK;
}

}  // namespace

extern "C" {

int fz_stream_open(fz_ctx *ctx, uint32_t mode, const uint8_t *p, uint32_t m, uint32_t max_subs, uint32_t max_ins,
                   uint32_t max_dels, uint32_t k, uint64_t seg_stride, uint32_t seg_pre, uint32_t seg_post,
                   uint64_t batch_bytes, fz_stream **out) {
    if (!out) return fail(FZ_EINVAL, "null argument");
    *out = nullptr;
    if (!ctx || ctx->devs.empty()) return fail(FZ_EINVAL, "bad ctx handle");
    if (ctx->devs.size() != 1) return fail(FZ_EUNSUPPORTED, "file streams run on a single-device context");
    if (ctx->npend || ctx->stream_inflight) return fail(FZ_EINVAL, "another search of this context is in flight");
    if (!p || m == 0) return fail(FZ_EINVAL, "subsequence must not be empty");
    if (m > FZ_MAX_M_ANY) return fail(FZ_EUNSUPPORTED, "subsequence longer than %u bytes", FZ_MAX_M_ANY);
    if (mode > FZ_MODE_GENERIC) return fail(FZ_EINVAL, "bad mode");
    if (mode == FZ_MODE_GENERIC && (uint64_t)m + 2ull * k > 65535ull)
        return fail(FZ_EUNSUPPORTED, "generic search: len(subsequence) + 2 * max_l_dist exceeds 65535 (16-bit window coordinates)");
    if (k > (mode == FZ_MODE_GENERIC ? (uint32_t)FZ_MAX_K : FZ_MAX_K_ANY)) return fail(FZ_EUNSUPPORTED, "distance limit %u is not supported", k);
    if (seg_stride == 0 || (seg_pre && seg_post)) return fail(FZ_EINVAL, "bad segment geometry");
    // a position may lie in at most two segments, and a chunk must hold a whole pattern window with its reach
    if ((uint64_t)seg_pre + seg_post > seg_stride / 2 || (uint64_t)m + 2ull * k + 2 > seg_stride)
        return fail(FZ_EUNSUPPORTED, "chunk too small for this pattern (use the per-chunk path)");
    fz_stream *st = new (std::nothrow) fz_stream();
    if (!st) return fail(FZ_ENOMEM, "out of memory");
    st->ctx = ctx;
    st->mode = mode; st->m = m; st->k = k;
    st->max_subs = std::min(max_subs, 255u); st->max_ins = std::min(max_ins, 255u); st->max_dels = std::min(max_dels, 255u);
    st->pat.assign(p, p + m);
    st->S = seg_stride; st->pre = seg_pre; st->post = seg_post;
    int rc = stream_build_search(st);
    if (rc) { delete st; return rc; }
    const uint64_t ext = (uint64_t)seg_pre + seg_post;
    st->cap = std::max<uint64_t>(batch_bytes, seg_stride + ext) + seg_stride + ext;   // >= one whole chunk + the carried overlap
    DevState &d = ctx->devs[0];
    auto init = [&]() -> int {
        HIP_TRY(hipSetDevice(d.device));
        const uint64_t need_d = FZ_PAD_FRONT + ((st->cap + FZ_TILE_BYTES - 1) / FZ_TILE_BYTES + 1) * FZ_TILE_BYTES + FZ_PAD_BACK;
        uint8_t *cached_d = nullptr;
        if (d.stream_h[0] && d.stream_cap >= st->cap && d.stream_d_bytes >= need_d) {       // reuse the previous stream's buffers
            st->h_buf[0] = d.stream_h[0]; st->h_buf[1] = d.stream_h[1];
            cached_d = d.stream_d;
            st->cap_alloc = d.stream_cap;
            d.stream_h[0] = d.stream_h[1] = nullptr; d.stream_d = nullptr;
        } else {
            for (int i = 0; i < 2; ++i) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&st->h_buf[i]), st->cap, hipHostMallocDefault));
            st->cap_alloc = st->cap;
        }
        st->seq = new (std::nothrow) fz_seq();
        if (!st->seq) return fail(FZ_ENOMEM, "out of memory");
        st->seq->ctx = ctx;
        st->seq->shards.emplace_back();
        Shard &sh = st->seq->shards[0];
        sh.dev = 0;
        if (cached_d) {
            sh.d_alloc = cached_d;
            sh.alloc_bytes = d.stream_d_bytes;
        } else {
            sh.alloc_bytes = need_d;
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sh.d_alloc), sh.alloc_bytes));
        }
        sh.d_buf = sh.d_alloc + FZ_PAD_FRONT;
        HIP_TRY(hipMemsetAsync(sh.d_alloc, 0, FZ_PAD_FRONT, d.stream));
        return FZ_OK;
    };
    rc = init();
    if (rc) { fz_stream_close(st); return rc; }
    *out = st;
    return FZ_OK;
}

int fz_stream_buffer(fz_stream *st, uint8_t **host, uint64_t *capacity) {
    if (!st || !host || !capacity) return fail(FZ_EINVAL, "null argument");
    *host = st->h_buf[st->cur] + st->stage_len;
    *capacity = st->eof ? 0 : st->cap - st->stage_len;
    return FZ_OK;
}

int fz_stream_submit(fz_stream *st, uint64_t nbytes, int last) {
    if (!st) return fail(FZ_EINVAL, "null argument");
    if (st->eof) return fail(FZ_EINVAL, "the stream has already seen its last bytes");
    if (nbytes > st->cap - st->stage_len) return fail(FZ_EINVAL, "more bytes than the staging buffer holds");
    st->stage_len += nbytes;
    st->bytes_total += nbytes;
    if (last) st->eof = true;
    const uint64_t data_end = st->stage_off + st->stage_len;
    const uint64_t ext_lo = st->pre, ext_hi = st->post;
    for (;;) {
        uint64_t j1;
        if (st->eof) j1 = stream_segments_at_eof(st, data_end);
        else j1 = data_end >= ext_hi + st->S ? (data_end - ext_hi) / st->S : 0;      // (j + 1) * S + post <= data_end
        if (j1 <= st->next_seg) {
            if (st->eof || st->stage_len < st->cap) break;
            return fail(FZ_EUNSUPPORTED, "staging buffer smaller than one chunk");
        }
        auto now = []() { return std::chrono::steady_clock::now(); };
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
            return std::chrono::duration<double, std::milli>(b - a).count();
        };
        const auto t0 = now();
        int rc = stream_collect(st);                        // the previous batch (its staging buffer becomes free)
        if (rc) return rc;
        const auto t1 = now();
        const uint64_t data_hi = st->eof ? data_end : j1 * st->S + ext_hi;
        rc = stream_launch(st, st->next_seg, j1, data_hi);
        if (rc) return rc;
        const auto t2 = now();
        st->t_collect += ms(t0, t1);
        st->t_launch += ms(t1, t2);
        st->next_seg = j1;
        if (st->eof) break;
        // carry the bytes the next segments need into the other staging buffer
        const uint64_t keep_from = j1 * st->S > ext_lo ? j1 * st->S - ext_lo : 0;
        const uint64_t from = std::max(keep_from, st->stage_off);
        const uint64_t carry = data_end - from;
        const int other = st->cur ^ 1;
        memcpy(st->h_buf[other], st->h_buf[st->cur] + (from - st->stage_off), carry);
        st->t_carry += ms(t2, now());
        st->cur = other;
        st->stage_off = from;
        st->stage_len = carry;
        break;
    }
    return FZ_OK;
}

namespace {

// Readers of fz_stream_read_fd: page cache -> pinned staging is a memcpy (one core moves ~5-10 GB/s, the PCIe link
// ~55).  The threads live for the whole file and take 1 MiB pieces of the current batch from a shared counter;
// starting and joining 16-48 threads for every 64 MiB batch cost ~0.5 ms of the batch's ~1.7 ms.
struct ReadPool {
    static constexpr uint64_t kPiece = 1u << 20;
    std::mutex mu;
    std::condition_variable go, done;
    uint64_t generation = 0;
    int busy = 0;
    bool stop = false;
    int fd = -1;
    uint8_t *dst = nullptr;
    uint64_t room = 0, pos = 0, npieces = 0;
    std::atomic<uint64_t> next{0};
    std::vector<uint64_t> got;           // bytes read per piece
    std::atomic<int> err{0};
    std::vector<std::thread> workers;

    explicit ReadPool(int n) {
        for (int t = 0; t < n; ++t) workers.emplace_back([this]() { run(); });
    }
    ~ReadPool() {
        { std::lock_guard<std::mutex> g(mu); stop = true; }
        go.notify_all();
        for (auto &w : workers) w.join();
    }
    void run() {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu);
                go.wait(lk, [&]() { return stop || generation != seen; });
                if (stop) return;
                seen = generation;
            }
            for (;;) {
                const uint64_t i = next.fetch_add(1, std::memory_order_relaxed);
                if (i >= npieces) break;
                const uint64_t lo = i * kPiece, hi = std::min(room, lo + kPiece);
                uint64_t n = 0;
                while (lo + n < hi) {
                    const ssize_t r = pread(fd, dst + lo + n, hi - lo - n, (off_t)(pos + lo + n));
                    if (r < 0) { err.store(1); break; }
                    if (r == 0) break;
                    n += (uint64_t)r;
                }
                got[i] = n;
            }
            std::lock_guard<std::mutex> g(mu);
            if (--busy == 0) done.notify_one();
        }
    }
    // fill dst[0, room) from the file at `pos`; -> bytes valid from the front (short at the end of the file)
    int fill(int fd_, uint8_t *dst_, uint64_t room_, uint64_t pos_, uint64_t &n, bool &short_read) {
        fd = fd_; dst = dst_; room = room_; pos = pos_;
        npieces = (room + kPiece - 1) / kPiece;
        got.assign(npieces, 0);
        next.store(0);
        {
            std::unique_lock<std::mutex> lk(mu);
            busy = (int)workers.size();
            ++generation;
            go.notify_all();
            done.wait(lk, [&]() { return busy == 0; });
        }
        if (err.load()) return fail(FZ_EDEVICE, "pread failed");
        n = 0;
        short_read = false;
        for (uint64_t i = 0; i < npieces && !short_read; ++i) {
            n += got[i];
            if (got[i] < std::min(room, (i + 1) * kPiece) - i * kPiece) short_read = true;   // end of file inside this piece
        }
        return FZ_OK;
    }
};

}  // namespace

int fz_stream_read_fd(fz_stream *st, int fd, int64_t offset, int threads, uint64_t *total) {
    if (!st || fd < 0 || offset < 0) return fail(FZ_EINVAL, "bad argument");
    if (threads <= 0) threads = (int)std::min<unsigned>(32u, std::max(1u, std::thread::hardware_concurrency() / 2));
    uint64_t pos = (uint64_t)offset, sum = 0;
    ReadPool pool(threads);
    while (!st->eof) {
        uint8_t *dst = nullptr;
        uint64_t room = 0;
        int rc = fz_stream_buffer(st, &dst, &room);
        if (rc) return rc;
        if (room == 0) return fail(FZ_EDEVICE, "internal: no staging room");
        uint64_t n = 0;
        bool short_read = false;
        const auto tf = std::chrono::steady_clock::now();
        rc = pool.fill(fd, dst, room, pos, n, short_read);
        if (rc) return rc;
        st->t_fill += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf).count();
        rc = fz_stream_submit(st, n, short_read ? 1 : 0);
        if (rc) return rc;
        pos += n;
        sum += n;
    }
    if (total) *total = sum;
    return FZ_OK;
}

int fz_stream_finish(fz_stream *st, fz_match **out, uint32_t **seg, uint64_t *n) {
    if (!st || !out || !seg || !n) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *seg = nullptr; *n = 0;
    if (!st->eof) {
        int rc = fz_stream_submit(st, 0, 1);
        if (rc) return rc;
    }
    int rc = stream_collect(st);
    if (rc) return rc;
    if (sw().stream_trace)
        fprintf(stderr, "[fz_stream] %.1f MiB: fill %.2f ms, collect %.2f ms, launch %.2f ms, carry %.2f ms\n",
                st->bytes_total / 1048576.0, st->t_fill, st->t_collect, st->t_launch, st->t_carry);
    void *mem = nullptr, *smem_ = nullptr;
    rc = alloc_out(st->out.size(), sizeof(fz_match), &mem);
    if (rc) return rc;
    rc = alloc_out(st->out_seg.size(), sizeof(uint32_t), &smem_);
    if (rc) { release_out(mem); return rc; }
    if (!st->out.empty()) {
        memcpy(mem, st->out.data(), st->out.size() * sizeof(fz_match));
        memcpy(smem_, st->out_seg.data(), st->out_seg.size() * sizeof(uint32_t));
    }
    *out = static_cast<fz_match *>(mem);
    *seg = static_cast<uint32_t *>(smem_);
    *n = st->out.size();
    st->out.clear();
    st->out_seg.clear();
    return FZ_OK;
}

void fz_stream_close(fz_stream *st) {
    if (!st) return;
    fz_ctx *ctx = st->ctx;
    if (ctx && !ctx->devs.empty()) {
        DevState &d = ctx->devs[0];
        (void)hipSetDevice(d.device);
        if (d.stream) (void)hipStreamSynchronize(d.stream);
        if (ctx->stream_inflight == st) ctx->stream_inflight = nullptr;
    }
    // hand the staging to the context for the next stream (freed with the context)
    bool kept = false;
    if (ctx && !ctx->devs.empty() && st->h_buf[0] && st->h_buf[1] && st->seq && !st->seq->shards.empty() && st->seq->shards[0].d_alloc) {
        DevState &d = ctx->devs[0];
        if (!d.stream_h[0] || d.stream_cap < st->cap_alloc) {
            for (int i = 0; i < 2; ++i) if (d.stream_h[i]) (void)hipHostFree(d.stream_h[i]);
            if (d.stream_d) (void)hipFree(d.stream_d);
            d.stream_h[0] = st->h_buf[0]; d.stream_h[1] = st->h_buf[1];
            d.stream_d = st->seq->shards[0].d_alloc;
            d.stream_cap = st->cap_alloc;
            d.stream_d_bytes = st->seq->shards[0].alloc_bytes;
            kept = true;
        }
    }
    if (!kept) {
        for (int i = 0; i < 2; ++i) if (st->h_buf[i]) (void)hipHostFree(st->h_buf[i]);
        if (st->seq) for (Shard &sh : st->seq->shards) if (sh.d_alloc) (void)hipFree(sh.d_alloc);
    }
    delete st->seq;
    delete st;
}

}  // extern "C"

namespace {

// Second stage of the consolidation: (hull, best match) pairs of connected sets of matches — from the host's run
// folding (fz_consolidate) or from the device's per-hit folding (fz_generic_ngrams_consolidated) — are ordered by
// (hull start, zero-length first) and a sweep merges overlapping hulls; the survivors are sorted by (start, end, dist).
int consolidate_hulls(std::vector<Hull> &hulls, fz_match **out, uint64_t *n_out) {
    auto by_start_end_dist = [](const fz_match &a, const fz_match &b) {
        if (a.start != b.start) return a.start < b.start;
        if (a.end != b.end) return a.end < b.end;
        if (a.dist != b.dist) return a.dist < b.dist;
        return a.block < b.block;                              // (equal matches of different n-gram hits: a fixed order)
    };
    auto better = [](const fz_match &x, const fz_match &y) {
        const int64_t lx = x.end - x.start, ly = y.end - y.start;
        return x.dist < y.dist || (x.dist == y.dist && (lx > ly || (lx == ly && (x.start < y.start || (x.start == y.start && x.block < y.block)))));
    };
    const uint64_t nh = hulls.size();
    if (nh > 0xffffffffull) return fail(FZ_EUNSUPPORTED, "more than 2^32 disjoint runs of matches");
    // Sweep order = (hull start, zero-length first, input order).  The hulls of a search are spread over the sequence
    // (one or a few per n-gram hit), so ONE counting pass over ~nh equal slices of [smin, smax] leaves almost every hull
    // alone in its slice: count, prefix, scatter the hull numbers, then one pass over the slices that fixes the order
    // inside the few holding several (stable insertion; a stable sort for the crowded slices of clustered input) and
    // sweeps.  (This replaces an 11-bit LSD radix over 64-bit words — a histogram pass and three scatter passes; moving
    // the 40-byte hulls themselves into the slices instead of their numbers measured slower.)
    static thread_local std::vector<uint32_t> order, cnt;       // hull numbers in sweep order; slice boundaries
    Trace trc;
    // The stream of an n-gram search arrives block-major with every block's rows in index order: the hulls are a handful
    // of ASCENDING RUNS (one per n-gram block).  Those are merged and swept in one sequential pass — no counting pass, no
    // scatter, no gathers in random order (configs[1], 2 409 rows: 40 -> ~15 us on the host).  Ties go to the earlier
    // run, which is the input order the sweep order asks for.
    {
        constexpr uint32_t kMaxRuns = 8;
        uint64_t head[kMaxRuns], end[kMaxRuns];
        uint32_t nruns = nh ? 1u : 0u;
        head[0] = 0;
        auto hull_before = [](const Hull &a, const Hull &b) {
            if (a.h0 != b.h0) return a.h0 < b.h0;
            return (a.h1 == a.h0) && (b.h1 != b.h0);
        };
        for (uint64_t i = 1; i < nh && nruns <= kMaxRuns; ++i)
            if (hull_before(hulls[i], hulls[i - 1])) {
                if (nruns < kMaxRuns) { end[nruns - 1] = i; head[nruns] = i; }
                ++nruns;
            }
        if (nruns && nruns <= kMaxRuns) {
            end[nruns - 1] = nh;
            void *mem = nullptr;
            int rc = alloc_out(nh, sizeof(fz_match), &mem);
            if (rc) return rc;
            fz_match *best = static_cast<fz_match *>(mem);
            uint64_t nbest = 0;
            int64_t h0 = 0, h1 = 0;
            for (;;) {
                uint32_t r = nruns;
                for (uint32_t c = 0; c < nruns; ++c)
                    if (head[c] < end[c] && (r == nruns || hull_before(hulls[head[c]], hulls[head[r]]))) r = c;
                if (r == nruns) break;
                const Hull &h = hulls[head[r]++];
                if (nbest && !(h.h1 <= h0 || h.h0 >= h1)) {
                    h0 = std::min(h0, h.h0);
                    h1 = std::max(h1, h.h1);
                    if (better(h.best, best[nbest - 1])) best[nbest - 1] = h.best;
                } else {
                    h0 = h.h0; h1 = h.h1;
                    best[nbest++] = h.best;
                }
            }
            trc.mark("  runs merged + sweep");
            if (!std::is_sorted(best, best + nbest, by_start_end_dist)) std::sort(best, best + nbest, by_start_end_dist);
            trc.mark("  final order");
            *out = best;
            *n_out = nbest;
            return FZ_OK;
        }
    }
    order.resize(nh);
    auto before = [&](uint32_t x, uint32_t y) {
        const Hull &a = hulls[x], &b = hulls[y];
        if (a.h0 != b.h0) return a.h0 < b.h0;
        return (a.h1 == a.h0) && (b.h1 != b.h0);
    };
    uint64_t nb = 1;
    if (nh >= 32) {
        int64_t smin = hulls[0].h0, smax = smin;
        for (const Hull &h : hulls) { smin = std::min(smin, h.h0); smax = std::max(smax, h.h0); }
        while (nb < nh && nb < (1u << 24)) nb <<= 1;
        const uint64_t range = (uint64_t)(smax - smin);
        int shift = 0;
        while ((range >> shift) >= nb) ++shift;
        cnt.assign(nb + 1, 0u);
        for (uint64_t i = 0; i < nh; ++i) ++cnt[(((uint64_t)(hulls[i].h0 - smin)) >> shift) + 1];
        for (uint64_t b = 1; b <= nb; ++b) cnt[b] += cnt[b - 1];                      // cnt[b] = where slice b starts
        for (uint64_t i = 0; i < nh; ++i) order[cnt[((uint64_t)(hulls[i].h0 - smin)) >> shift]++] = (uint32_t)i;
        // now cnt[b] = where slice b ends
    } else {
        for (uint64_t i = 0; i < nh; ++i) order[i] = (uint32_t)i;
        std::stable_sort(order.begin(), order.end(), before);
        cnt.assign(1, (uint32_t)nh);
    }
    trc.mark("  hulls in slices");
    // the survivors go straight into the caller's buffer (at most one per hull)
    void *mem = nullptr;
    int rc = alloc_out(nh, sizeof(fz_match), &mem);
    if (rc) return rc;
    fz_match *best = static_cast<fz_match *>(mem);
    uint64_t nbest = 0;
    int64_t h0 = 0, h1 = 0;
    uint32_t lo = 0;
    for (uint64_t b = 0; b < nb; ++b) {
        const uint32_t hi = cnt[b];
        if (hi - lo > 1 && nh >= 32) {
            if (hi - lo > 24) std::stable_sort(order.begin() + lo, order.begin() + hi, before);
            else
                for (uint32_t i = lo + 1; i < hi; ++i) {
                    const uint32_t v = order[i];
                    uint32_t j = i;
                    while (j > lo && before(v, order[j - 1])) { order[j] = order[j - 1]; --j; }
                    order[j] = v;
                }
        }
        for (uint32_t vi = lo; vi < hi; ++vi) {
            if (vi + 12 < nh) __builtin_prefetch(&hulls[order[vi + 12]]);    // (the hulls are gathered in random order)
            const Hull &h = hulls[order[vi]];
            if (nbest && !(h.h1 <= h0 || h.h0 >= h1)) {
                h0 = std::min(h0, h.h0);
                h1 = std::max(h1, h.h1);
                if (better(h.best, best[nbest - 1])) best[nbest - 1] = h.best;
            } else {
                h0 = h.h0; h1 = h.h1;
                best[nbest++] = h.best;
            }
        }
        lo = hi;
    }
    trc.mark("  sweep");
    if (!std::is_sorted(best, best + nbest, by_start_end_dist)) std::sort(best, best + nbest, by_start_end_dist);
    trc.mark("  final order");
    *out = best;
    *n_out = nbest;
    return FZ_OK;
}

}  // namespace

extern "C" {

// ---- host-side consolidation (common.py:145-189) -------------------------------------------
// The partition into overlap groups is input-order independent, so for
// fz_consolidate a sort + sweep replaces the reference's O(M * groups) loop.
int fz_consolidate(const fz_match *in, uint64_t n, fz_match **out, uint64_t *n_out) {
    if (!out || !n_out || (!in && n)) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *n_out = 0;
    // Two stages.  (1) One pass in input order folds every row that overlaps the running hull of the rows right
    // before it into that hull (the reference's own group test, common.py:150-159, applied to consecutive rows;
    // the partition is order independent).  The records of one n-gram hit are emitted back to back and nearly all
    // overlap, so the 2.1e5 rows of configs[3b] leave ~6e3 (hull, best row) pairs; streams without such runs pass
    // through unchanged.  (2) The pairs are ordered by (hull start, zero-length first) — 11-bit LSD radix passes on
    // one 64-bit word per pair when there are many, a comparison sort otherwise (2e5 24-byte rows: ~6 ms) — and a
    // sweep merges overlapping hulls.  Zero-length matches (start == end) never overlap anything under
    // `not (end <= g.start or start >= g.end)` unless strictly inside a group, so both stages use that predicate
    // against the running hull instead of assuming sorted-interval merging.
    auto better = [](const fz_match &x, const fz_match &y) {
        const int64_t lx = x.end - x.start, ly = y.end - y.start;
        return x.dist < y.dist || (x.dist == y.dist && (lx > ly || (lx == ly && (x.start < y.start || (x.start == y.start && x.block < y.block)))));
    };
    static thread_local std::vector<Hull> hulls;                // scratch kept per thread between calls
    hulls.clear();
    Trace trc;
    for (uint64_t i = 0; i < n; ++i) {
        const fz_match &mt = in[i];
        if (!hulls.empty()) {
            Hull &h = hulls.back();
            if (!(mt.end <= h.h0 || mt.start >= h.h1)) {
                h.h0 = std::min(h.h0, mt.start);
                h.h1 = std::max(h.h1, mt.end);
                if (better(mt, h.best)) h.best = mt;
                continue;
            }
        }
        hulls.push_back(Hull{mt.start, mt.end, mt});
    }
    trc.mark("  runs folded");
    return consolidate_hulls(hulls, out, n_out);
}

int fz_merge_ranks(const fz_match *const *parts, const uint64_t *counts, const uint64_t *block_counts,
                   uint32_t world, uint32_t nb, fz_match *out) {
    if (!parts || !counts || !block_counts || !out) return fail(FZ_EINVAL, "null argument");
    std::vector<uint64_t> pos(world, 0);                       // read position inside every rank's stream
    for (uint32_t r = 0; r < world; ++r) {
        uint64_t sum = 0;
        for (uint32_t g = 0; g < nb; ++g) sum += block_counts[(size_t)r * nb + g];
        if (sum != counts[r]) return fail(FZ_EINVAL, "rank %u: block counts do not add up to its record count", r);
    }
    uint64_t o = 0;
    for (uint32_t g = 0; g < nb; ++g)
        for (uint32_t r = 0; r < world; ++r) {
            const uint64_t c = block_counts[(size_t)r * nb + g];
            if (c) memcpy(out + o, parts[r] + pos[r], c * sizeof(fz_match));
            o += c;
            pos[r] += c;
        }
    return FZ_OK;
}

namespace {
struct WireRow { int64_t start; uint32_t len; uint16_t dist; uint16_t block; };
struct WireHeader { uint64_t count, nblocks; uint32_t per_block[256]; };
static_assert(sizeof(WireRow) == 16 && sizeof(WireHeader) == FZ_WIRE_HEADER_ROWS * 16, "wire layout");
}  // namespace

int fz_wire_pack(const fz_match *in, uint64_t n, uint64_t cap_rows, void *dst) {
    if ((!in && n) || !dst) return fail(FZ_EINVAL, "null argument");
    WireHeader *h = static_cast<WireHeader *>(dst);
    WireRow *rows = reinterpret_cast<WireRow *>(h + 1);
    memset(h, 0, sizeof *h);
    h->count = n;
    const uint64_t fit = std::min(n, cap_rows);
    uint32_t nb = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const int32_t b = in[i].block;
        if (b < 0 || b > 255 || in[i].end < in[i].start || in[i].end - in[i].start > 0xffffffffll || in[i].dist < 0 ||
            in[i].dist > 0xffff)
            return fail(FZ_EUNSUPPORTED, "record %llu does not fit the torch glue's wire format (at most 256 n-gram blocks, i.e. max_l_dist "
                        "< 256, 32-bit lengths, 16-bit distances): use the native collective (fz_comm_*), which has no such limit",
                        (unsigned long long)i);
        ++h->per_block[b];
        nb = std::max(nb, (uint32_t)b + 1);
        if (i < fit) rows[i] = WireRow{in[i].start, (uint32_t)(in[i].end - in[i].start), (uint16_t)in[i].dist, (uint16_t)b};
    }
    h->nblocks = nb;
    return FZ_OK;
}

int fz_wire_merge(const void *recv, uint32_t world, uint64_t rows_per_rank, uint64_t cap_rows,
                  fz_match *out, uint64_t out_cap, uint64_t *n_out, uint64_t *max_count) {
    if (!recv || !n_out || !max_count || rows_per_rank < FZ_WIRE_HEADER_ROWS + cap_rows) return fail(FZ_EINVAL, "bad argument");
    const uint8_t *base = static_cast<const uint8_t *>(recv);
    uint64_t total = 0, top = 0;
    uint32_t nb = 0;
    for (uint32_t r = 0; r < world; ++r) {
        const WireHeader *h = reinterpret_cast<const WireHeader *>(base + (size_t)r * rows_per_rank * 16);
        if (h->nblocks > 256) return fail(FZ_EINVAL, "rank %u: corrupt header", r);
        total += h->count;
        top = std::max(top, h->count);
        nb = std::max(nb, (uint32_t)h->nblocks);
    }
    *n_out = total;
    *max_count = top;
    if (top > cap_rows) return FZ_OK;                          // caller re-gathers with a larger capacity
    if (total > out_cap || (total && !out)) return fail(FZ_EINVAL, "output too small for %llu records", (unsigned long long)total);
    std::vector<uint64_t> pos(world, 0);
    uint64_t o = 0;
    for (uint32_t g = 0; g < nb; ++g)
        for (uint32_t r = 0; r < world; ++r) {
            const WireHeader *h = reinterpret_cast<const WireHeader *>(base + (size_t)r * rows_per_rank * 16);
            const WireRow *rows = reinterpret_cast<const WireRow *>(h + 1) + pos[r];
            const uint32_t c = h->per_block[g];
            if (pos[r] + c > h->count) return fail(FZ_EINVAL, "rank %u: block counts exceed its record count", r);
            for (uint32_t i = 0; i < c; ++i, ++o) {
                out[o].start = rows[i].start;
                out[o].end = rows[i].start + (int64_t)rows[i].len;
                out[o].dist = rows[i].dist;
                out[o].block = rows[i].block;
            }
            pos[r] += c;
        }
    return FZ_OK;
}

int fz_debug_order_records(const void *recs, uint64_t n, uint32_t L, fz_match **out, uint64_t *n_out) {
    if ((!recs && n) || !out || !n_out) return fail(FZ_EINVAL, "null argument");
    static_assert(sizeof(FzRec) == 24, "record layout");
    return emit_matches(static_cast<const FzRec *>(recs), (size_t)n, L, out, n_out);
}

int fz_debug_order_records_bounded(const void *recs, uint64_t n, uint32_t L, uint64_t idx_bound, uint32_t blk_bound,
                                   fz_match **out, uint64_t *n_out) {
    if ((!recs && n) || !out || !n_out || !idx_bound || !blk_bound) return fail(FZ_EINVAL, "null argument");
    return emit_matches(static_cast<const FzRec *>(recs), (size_t)n, L, out, n_out, idx_bound, blk_bound, /*may_have_empty=*/true);
}

int fz_debug_order_segments(const void *recs, const uint64_t *seg_ends, uint32_t n_segments, uint32_t L, fz_match **out, uint64_t *n_out) {
    if ((!recs && n_segments) || !seg_ends || !out || !n_out || n_segments == 0) return fail(FZ_EINVAL, "null argument");
    std::vector<size_t> ends(seg_ends, seg_ends + n_segments);
    std::vector<uint32_t> order(n_segments);
    for (uint32_t i = 0; i < n_segments; ++i) order[i] = i;
    return emit_matches_segments(nullptr, static_cast<const FzRec *>(recs), ends, order, L, out, n_out, 0, 0, true);
}

int fz_debug_launch_plan(const uint8_t *p, uint32_t m, uint32_t L, uint32_t *out, uint32_t cap, uint32_t *n_launches) {
    if (!p || !out || !n_launches || L == 0 || L > m) return fail(FZ_EINVAL, "bad argument");
    std::vector<uint32_t> starts;
    for (uint32_t s = 0; s + L <= m; s += L) starts.push_back(s);
    const uint32_t G = (uint32_t)starts.size();
    uint32_t nl = 0;
    for (uint32_t g0 = 0; g0 < G;) {
        uint32_t hk = 0, sh = 0;
        const uint32_t nb = choose_launch_blocks(p, starts.data(), g0, G, L, hk, sh);
        if (nb == 0) return fail(FZ_EDEVICE, "internal: a launch without blocks");
        if (nl < cap) { out[4 * nl] = g0; out[4 * nl + 1] = nb; out[4 * nl + 2] = hk; out[4 * nl + 3] = sh; }
        ++nl;
        g0 += nb;
    }
    *n_launches = nl;
    return FZ_OK;
}

// Faithful group-list-order version (common.py:161-177), needed by the substitutions-only path: a match joins
// the group(s) whose hull it overlaps; one group is extended in place, several are removed and their union is
// appended at the END of the list; the result is in final list order.  The reference tests every group for
// every match (O(M * groups): 2 ms for the 2e3 raw matches of configs[2], 50 ms for 2e4).  Group hulls never
// overlap each other (a match that would make two hulls overlap overlaps both groups and merges them; a
// zero-length group is a point that is never strictly inside another hull), so the groups are kept ordered by
// (hull start, hull end) and the groups a match overlaps are a contiguous run found by one search; the list
// position of a group is a sequence number handed out on creation and on merges.
static int group_best_exact(const fz_match *in, uint64_t n, fz_match **out, uint64_t *n_out);

// Fast form for what the searches produce (round 4: the std::map walk below cost 0.39 ms on the 2.8e3 rows of configs[2],
// more than the search it follows): thousands of matches in a few hundred to a few thousand SMALL groups.  The partition
// into groups is order independent (connected components of the overlap relation: sort + sweep, as fz_consolidate);
// what depends on the input order is only WHERE in the list a group ends up, and that is decided inside the group: a
// group's position is the moment (input index) of the last event that gave it a new list entry — its creation, or the
// last merge of two or more groups into one (the union is appended at the end, common.py:169-175); extensions in place
// keep the entry.  So every component replays its own members in input order on a handful of sub-groups, and the
// components are emitted in the order of those moments.  Components with many members (dense repeats) or anything the
// sweep and the replay disagree on take the exact walk.
int fz_group_best(const fz_match *in, uint64_t n, fz_match **out, uint64_t *n_out) {
    if (!out || !n_out || (!in && n)) return fail(FZ_EINVAL, "null argument");
    *out = nullptr; *n_out = 0;
    if (n < 32 || n > 0x7fffffffull) return group_best_exact(in, n, out, n_out);
    auto better = [](const fz_match &a, const fz_match &b) {
        const int64_t la = a.end - a.start, lb = b.end - b.start;
        return a.dist < b.dist || (a.dist == b.dist && (la > lb || (la == lb && a.start < b.start)));
    };
    static thread_local std::vector<uint32_t> order, cnt, comp, first, members, slot;
    // (1) sweep order = (start, zero-length first, input order): one counting pass over ~n slices of the start range,
    //     then the few crowded slices are fixed (as consolidate_hulls does)
    order.resize(n);
    int64_t smin = in[0].start, smax = smin;
    for (uint64_t i = 0; i < n; ++i) { smin = std::min(smin, in[i].start); smax = std::max(smax, in[i].start); }
    uint64_t nb = 1;
    while (nb < n && nb < (1u << 24)) nb <<= 1;
    const uint64_t range = (uint64_t)(smax - smin);
    int shift = 0;
    while ((range >> shift) >= nb) ++shift;
    cnt.assign(nb + 1, 0u);
    for (uint64_t i = 0; i < n; ++i) ++cnt[(((uint64_t)(in[i].start - smin)) >> shift) + 1];
    for (uint64_t b = 1; b <= nb; ++b) cnt[b] += cnt[b - 1];
    for (uint64_t i = 0; i < n; ++i) order[cnt[((uint64_t)(in[i].start - smin)) >> shift]++] = (uint32_t)i;
    auto before = [&](uint32_t x, uint32_t y) {
        const fz_match &a = in[x], &b = in[y];
        if (a.start != b.start) return a.start < b.start;
        const bool pa = a.end == a.start, pb = b.end == b.start;
        if (pa != pb) return pa;
        return x < y;
    };
    // (2) components
    comp.resize(n);
    uint32_t ncomp = 0, lo = 0, biggest = 0, cur = 0;
    int64_t h0 = 0, h1 = 0;
    for (uint64_t b = 0; b < nb; ++b) {
        const uint32_t hi = cnt[b];
        if (hi - lo > 1) {
            if (hi - lo > 24) std::sort(order.begin() + lo, order.begin() + hi, before);
            else
                for (uint32_t i = lo + 1; i < hi; ++i) {
                    const uint32_t v = order[i];
                    uint32_t j = i;
                    while (j > lo && before(v, order[j - 1])) { order[j] = order[j - 1]; --j; }
                    order[j] = v;
                }
        }
        for (uint32_t vi = lo; vi < hi; ++vi) {
            const fz_match &mt = in[order[vi]];
            if (ncomp && !(mt.end <= h0 || mt.start >= h1)) {
                h0 = std::min(h0, mt.start);
                h1 = std::max(h1, mt.end);
                biggest = std::max(biggest, ++cur);
            } else {
                h0 = mt.start; h1 = mt.end;
                ++ncomp;
                cur = 1;
            }
            comp[order[vi]] = ncomp - 1;
        }
        lo = hi;
    }
    if (biggest > 256) return group_best_exact(in, n, out, n_out);
    // (3) members of every component in input order
    first.assign((size_t)ncomp + 1, 0u);
    for (uint64_t i = 0; i < n; ++i) ++first[comp[i] + 1];
    for (uint32_t c = 0; c < ncomp; ++c) first[c + 1] += first[c];
    members.resize(n);
    {
        static thread_local std::vector<uint32_t> fill;
        fill.assign(first.begin(), first.end() - 1);
        for (uint64_t i = 0; i < n; ++i) members[fill[comp[i]]++] = (uint32_t)i;
    }
    // (4) replay every component; slot[moment] = component + 1
    slot.assign(n, 0u);
    struct Sub { int64_t s, e; uint32_t when; };
    Sub subs[260];
    for (uint32_t c = 0; c < ncomp; ++c) {
        const uint32_t b0 = first[c], b1 = first[c + 1];
        if (b1 - b0 == 1) { slot[members[b0]] = c + 1; continue; }
        uint32_t ns = 0;
        for (uint32_t q = b0; q < b1; ++q) {
            const uint32_t i = members[q];
            const fz_match &mt = in[i];
            uint32_t nov = 0, firstov = 0;
            for (uint32_t g = 0; g < ns; ++g)
                if (!(mt.end <= subs[g].s || mt.start >= subs[g].e)) { if (!nov) firstov = g; ++nov; }
            if (nov == 0) {
                subs[ns++] = Sub{mt.start, mt.end, i};
            } else if (nov == 1) {
                subs[firstov].s = std::min(subs[firstov].s, mt.start);
                subs[firstov].e = std::max(subs[firstov].e, mt.end);
            } else {
                Sub u{mt.start, mt.end, i};
                uint32_t w = 0;
                for (uint32_t g = 0; g < ns; ++g) {
                    if (!(mt.end <= subs[g].s || mt.start >= subs[g].e)) {
                        u.s = std::min(u.s, subs[g].s);
                        u.e = std::max(u.e, subs[g].e);
                    } else {
                        subs[w++] = subs[g];
                    }
                }
                subs[w++] = u;
                ns = w;
            }
        }
        if (ns != 1) return group_best_exact(in, n, out, n_out);     // the sweep saw one component, the replay did not
        slot[subs[0].when] = c + 1;
    }
    void *mem = nullptr;
    int rc = alloc_out(ncomp, sizeof(fz_match), &mem);
    if (rc) return rc;
    fz_match *o = static_cast<fz_match *>(mem);
    uint64_t w = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (!slot[i]) continue;
        const uint32_t c = slot[i] - 1;
        fz_match best = in[members[first[c]]];
        for (uint32_t q = first[c] + 1; q < first[c + 1]; ++q)
            if (better(in[members[q]], best)) best = in[members[q]];
        o[w++] = best;
    }
    *out = o;
    *n_out = w;
    return FZ_OK;
}

static int group_best_exact(const fz_match *in, uint64_t n, fz_match **out, uint64_t *n_out) {
    struct Key {
        int64_t s, e; uint64_t seq;
        bool operator<(const Key &o) const { return s != o.s ? s < o.s : (e != o.e ? e < o.e : seq < o.seq); }
    };
    auto better = [](const fz_match &a, const fz_match &b) {
        const int64_t la = a.end - a.start, lb = b.end - b.start;
        return a.dist < b.dist || (a.dist == b.dist && (la > lb || (la == lb && a.start < b.start)));
    };
    std::map<Key, fz_match> groups;                            // key: hull + list position, value: best match
    uint64_t next_seq = 0;
    std::vector<std::map<Key, fz_match>::iterator> ov;
    for (uint64_t i = 0; i < n; ++i) {
        const fz_match &mt = in[i];
        auto overlaps = [&](const Key &g) { return !(mt.end <= g.s || mt.start >= g.e); };
        ov.clear();
        auto it = groups.lower_bound(Key{mt.start, INT64_MIN, 0});     // first group starting at or after the match
        // before it: points cannot overlap (they lie left of the match's start), and of the groups with a length
        // only the nearest one can reach across the match's start
        for (auto pb = it; pb != groups.begin();) {
            --pb;
            if (pb->first.e == pb->first.s) continue;
            if (overlaps(pb->first)) ov.push_back(pb);
            break;
        }
        for (; it != groups.end() && it->first.s < mt.end; ++it)
            if (overlaps(it->first)) ov.push_back(it);
        if (ov.empty()) {
            groups.emplace(Key{mt.start, mt.end, next_seq++}, mt);
        } else if (ov.size() == 1 && mt.start >= ov[0]->first.s && mt.end <= ov[0]->first.e) {
            if (better(mt, ov[0]->second)) ov[0]->second = mt;   // inside the hull (cross-block duplicates): nothing moves
        } else if (ov.size() == 1) {                           // extended in place: same list position
            auto node = groups.extract(ov[0]);
            node.key().s = std::min(node.key().s, mt.start);
            node.key().e = std::max(node.key().e, mt.end);
            if (better(mt, node.mapped())) node.mapped() = mt;
            groups.insert(std::move(node));
        } else {                                               // union appended at the end of the list
            std::sort(ov.begin(), ov.end(), [](const auto &x, const auto &y) { return x->first.seq < y->first.seq; });
            Key u{mt.start, mt.end, 0};
            fz_match best = mt;
            for (auto g : ov) {
                u.s = std::min(u.s, g->first.s);
                u.e = std::max(u.e, g->first.e);
                if (better(g->second, best)) best = g->second;
            }
            for (auto g : ov) groups.erase(g);
            u.seq = next_seq++;
            groups.emplace(u, best);
        }
    }
    std::vector<std::pair<uint64_t, fz_match>> ordered;
    ordered.reserve(groups.size());
    for (const auto &g : groups) ordered.emplace_back(g.first.seq, g.second);
    std::sort(ordered.begin(), ordered.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
    void *mem = nullptr;
    int rc = alloc_out(ordered.size(), sizeof(fz_match), &mem);
    if (rc) return rc;
    fz_match *o = static_cast<fz_match *>(mem);
    for (size_t g = 0; g < ordered.size(); ++g) o[g] = ordered[g].second;
    *out = o;
    *n_out = ordered.size();
    return FZ_OK;
}

int fz_set_timing(fz_ctx *ctx, int on) {
    if (!ctx) return fail(FZ_EINVAL, "null argument");
    if (ctx->npend || ctx->stream_inflight) return fail(FZ_EINVAL, "a search of this context is in flight");
    ctx->timing = on != 0;
    return FZ_OK;
}

int fz_set_scan_direction(fz_ctx *ctx, int mode) {
    if (!ctx || mode < 0 || mode > 2) return fail(FZ_EINVAL, "scan direction must be 0 (alternate), 1 (forward) or 2 (reversed)");
    if (ctx->npend || ctx->stream_inflight) return fail(FZ_EINVAL, "a search of this context is in flight");
    ctx->scan_dir = mode;
    return FZ_OK;
}

int fz_set_streams(fz_ctx *ctx, int n) {
    if (!ctx || (n != 1 && n != 2)) return fail(FZ_EINVAL, "streams must be 1 or 2");
    if (ctx->npend || ctx->stream_inflight) return fail(FZ_EINVAL, "a search of this context is in flight");
    ctx->streams = n;
    return FZ_OK;
}

int fz_stats(fz_ctx *ctx, fz_stats_t *out) {
    if (!ctx || !out) return fail(FZ_EINVAL, "null argument");
    resolve_timing(ctx);
    *out = ctx->stats;
    return FZ_OK;
}

int fz_mem_info(fz_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes) {
    if (!ctx || !free_bytes || !total_bytes) return fail(FZ_EINVAL, "null argument");
    uint64_t fmin = ~0ull, tmin = ~0ull;
    for (const DevState &d : ctx->devs) {
        HIP_TRY(hipSetDevice(d.device));
        size_t f = 0, t = 0;
        HIP_TRY(hipMemGetInfo(&f, &t));
        fmin = std::min<uint64_t>(fmin, f);
        tmin = std::min<uint64_t>(tmin, t);
    }
    *free_bytes = fmin;
    *total_bytes = tmin;
    return FZ_OK;
}

void fz_free(void *p) { release_out(p); }


}  // extern "C"
