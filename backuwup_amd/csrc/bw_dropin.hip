// bw_dropin.hip -- the two-`use`-line integration: the entry points behind the Rust
// drop-ins for `fastcdc::v2020::FastCDC` and `blake3::hash`, called the way the reference calls the
// crates, one task per file from tokio's worker threads (dir_packer.rs:166):
//
//   * CDC files (dir_packer.rs:254-266, then :286 per chunk): bw_fastcdc_chunks_hashed chunks AND
//     hashes the file in one submit and keeps the chunk digests under a handle; the per-chunk
//     blake3::hash drop-in (bw_blake3_hash_dropin) finds its digest there by (pointer, length) while
//     the handle lives.  The registry is an ordered map of the live sources (an interval lookup under
//     a reader lock) with a per-thread cache of the last source hit, so callers on many threads do
//     not serialize on one mutex and a lookup does not scan every open file.
//   * whole-file blobs and tree blobs (dir_packer.rs:267-271 -> :286, :274 -> :320/:353): one small
//     message per call.  Messages of at most 64 KiB go to the device's hash service (below): the
//     caller copies its message into pinned memory of its own and posts it into a ring of slots that
//     a persistent kernel's workers poll, and the digest comes back into the slot -- no launch per
//     call.  (The round-5 coalescer, kept as the BW_DROPIN_SERVICE=0 alternative, batched concurrent
//     calls into launches over four lanes; it paid ~20 us of launch, event and thread hand-offs per
//     batch.)  Larger messages run through the caller's own context (the batch pipeline, in parallel
//     across the callers' contexts): gathered into one library thread they measured 30 GB/s on C1
//     against 55 through the callers' own contexts.
//
// Only bw_blake3_hash_dropin consults the kept digests: its caller guarantees that the bytes under a
// live handle do not change (the Rust FastCDC drop-in borrows the mmap immutably for the handle's
// lifetime).  bw_blake3_hash always hashes the bytes it is given (a rewritten buffer must
// never be answered from an earlier chunking).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <linux/futex.h>
#include <immintrin.h>
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

#include "bw_internal.h"
#include "bw_b3_small.h"

using namespace bw;

namespace {

// ------------------------------------------------------------------ kept chunk digests
struct Kept {
    uint64_t handle;
    const uint8_t* base;
    uint64_t len;
    std::vector<uint64_t> off, clen;  // chunk offsets (ascending) and lengths
    std::vector<uint8_t> dig;         // 32 B per chunk
    std::atomic<bool> live{true};
};

std::shared_mutex g_kept_mu;
// live sources by base address (several handles may share a base: the vector); a lookup takes the
// greatest base <= the pointer and walks down while the ranges could still contain it
std::map<uintptr_t, std::vector<std::shared_ptr<Kept>>> g_kept_by_base;
std::map<uint64_t, std::shared_ptr<Kept>> g_kept_by_handle;
std::atomic<uint64_t> g_kept_next{1}, g_kept_hits{0};
uint64_t g_kept_maxlen = 0;  // the longest live source: bounds the walk down from the greatest base
thread_local std::weak_ptr<Kept> t_last;

bool answer(const Kept& k, const uint8_t* data, uint64_t len, uint8_t out[32]) {
    if (!k.live.load(std::memory_order_acquire) || data < k.base || data >= k.base + k.len) return false;
    const uint64_t o = (uint64_t)(data - k.base);
    auto it = std::lower_bound(k.off.begin(), k.off.end(), o);
    if (it == k.off.end() || *it != o) return false;
    const size_t i = it - k.off.begin();
    if (k.clen[i] != len) return false;
    memcpy(out, k.dig.data() + 32 * i, 32);
    return true;
}

bool kept_lookup(const uint8_t* data, uint64_t len, uint8_t out[32]) {
    if (auto k = t_last.lock())  // the task's own file, almost always
        if (answer(*k, data, len, out)) {
            g_kept_hits.fetch_add(1, std::memory_order_relaxed);
            return true;
        }
    std::shared_lock<std::shared_mutex> lk(g_kept_mu);
    if (g_kept_by_base.empty()) return false;
    auto it = g_kept_by_base.upper_bound((uintptr_t)data);
    while (it != g_kept_by_base.begin()) {
        --it;
        if ((uintptr_t)data - it->first >= g_kept_maxlen) break;  // no live source reaches this far
        for (const auto& k : it->second)
            if (answer(*k, data, len, out)) {
                t_last = k;
                g_kept_hits.fetch_add(1, std::memory_order_relaxed);
                return true;
            }
    }
    return false;
}

// ------------------------------------------------------------------ coalesced small messages
constexpr uint64_t CO_MAX_MSG = BW_COALESCE_MAX_MSG;  // larger messages go through the caller's context
static_assert(CO_MAX_MSG == B3_MSG_MAX, "a coalesced batch is one k_b3_msgs launch");
constexpr uint32_t CO_MAX_N = 1u << 16;         // messages per batch
// a batch's table in pinned memory: message addresses, lengths and digests (the small-message
// kernel reads and writes them there, over PCIe)
constexpr uint64_t CO_META = (uint64_t)CO_MAX_N * (8 + 8 + 32);
constexpr int CO_LANES = 4;                     // batches on the GPU at once, a stream each
constexpr int CO_BUFS = CO_LANES + 2;           // tables: in flight, filling, being read

// Each calling thread copies its message into pinned memory of its own before it joins a batch, so
// a batch is complete the moment it is closed: the launcher never waits for a caller that was
// descheduled between reserving room and finishing its copy (with 256 threads on 16 cores it
// waited milliseconds).  The buffer is reused by the thread's next call, after this one returned.
struct TlStage {
    uint8_t* p = nullptr;
    uint64_t cap = 0;
    ~TlStage() {
        if (p) hipHostFree(p);
    }
};
thread_local TlStage t_stage;

struct CoBatch {
    int buf = -1, lane = -1;
    uint8_t* meta = nullptr;
    uint64_t maxlen = 0;
    uint32_t n = 0;
    std::atomic<uint32_t> readers{0};
    std::vector<uint64_t> ptr, len;  // message addresses (each caller's pinned copy) and lengths
    const uint8_t* digp = nullptr;   // the digests (the table's digest area)
    bool sync = false;               // the launch failed: nothing to wait for
    int rc = 0;
    std::mutex mu;                   // its waiters
    std::condition_variable cv;
    bool done = false;
};

// One per device.  Callers add their message to the open batch; a launcher thread closes the open
// batch as soon as a lane is free and launches it; a completer thread waits for the launched batches
// in order and wakes their waiters.  Under load the open batch fills while every lane is busy (group
// commit); idle, a lone call is launched at once.  (Measured against letting the callers launch and
// complete their own batches: the library threads win once the callers outnumber the cores, where a
// caller that owns a finished batch waits for a core before it can hand its lane on.)
struct Combiner {
    int device = 0;
    std::mutex mu;
    std::condition_variable cv_work, cv_done, cv_room;
    bw_ctx* ctx[CO_LANES] = {};  // a lane's context: its stream
    hipEvent_t ev[CO_LANES] = {};
    bool lane_busy[CO_LANES] = {};
    uint8_t* bufs[CO_BUFS] = {};
    bool buf_busy[CO_BUFS] = {};
    std::shared_ptr<CoBatch> open;
    std::vector<std::shared_ptr<CoBatch>> launched;  // FIFO
    std::atomic<uint64_t> batches{0}, messages{0};
};

std::mutex g_co_mu;
Combiner* g_co[64] = {};

void launcher(Combiner* co) {
    hipSetDevice(co->device);
    std::unique_lock<std::mutex> lk(co->mu);
    for (;;) {
        int lane = -1;
        for (;;) {
            lane = -1;
            for (int k = 0; k < CO_LANES; k++)
                if (!co->lane_busy[k]) lane = k;
            if (lane >= 0 && co->open && co->open->n) break;
            co->cv_work.wait(lk);
        }
        std::shared_ptr<CoBatch> b = std::move(co->open);
        co->open.reset();
        co->lane_busy[lane] = true;
        b->lane = lane;
        co->cv_room.notify_all();  // callers waiting for room open the next batch
        lk.unlock();
        {
            // every message fits one wave: one launch reads them from the callers' pinned copies and
            // writes the digests into the batch's pinned table (no copy operations, no batch tables)
            uint64_t* ptrs = (uint64_t*)b->meta;
            uint64_t* lens = ptrs + CO_MAX_N;
            uint8_t* dig = (uint8_t*)(lens + CO_MAX_N);
            memcpy(ptrs, b->ptr.data(), 8ull * b->n);
            memcpy(lens, b->len.data(), 8ull * b->n);
            hipStream_t st = (hipStream_t)bw_get_stream(co->ctx[lane]);
            launch_b3_msgs(st, nullptr, ptrs, lens, b->n, (uint32_t)b->maxlen, dig);
            const hipError_t e = hipGetLastError();
            if (e == hipSuccess) hipEventRecord(co->ev[lane], st);
            b->rc = e == hipSuccess ? BW_OK : BW_EHIP;
            b->sync = e != hipSuccess;
            b->digp = dig;
        }
        co->batches.fetch_add(1, std::memory_order_relaxed);
        co->messages.fetch_add(b->n, std::memory_order_relaxed);
        lk.lock();
        co->launched.push_back(std::move(b));
        co->cv_done.notify_one();
    }
}

void completer(Combiner* co) {
    hipSetDevice(co->device);
    std::unique_lock<std::mutex> lk(co->mu);
    for (;;) {
        while (co->launched.empty()) co->cv_done.wait(lk);
        std::shared_ptr<CoBatch> b = co->launched.front();
        lk.unlock();
        if (!b->sync && hipEventSynchronize(co->ev[b->lane]) != hipSuccess) b->rc = BW_EHIP;
        {
            std::lock_guard<std::mutex> bl(b->mu);
            b->done = true;
        }
        b->cv.notify_all();
        lk.lock();
        co->launched.erase(co->launched.begin());
        co->lane_busy[b->lane] = false;
        co->cv_work.notify_one();
    }
}

Combiner* combiner(int device) {
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> lk(g_co_mu);
    if (!g_co[device]) {
        // lives as long as the process (the drop-ins have no teardown call), and so do its threads
        auto* c = new Combiner();
        c->device = device;
        hipSetDevice(device);
        for (int k = 0; k < CO_LANES; k++)
            if (bw_create(device, &c->ctx[k]) != BW_OK ||
                hipEventCreateWithFlags(&c->ev[k], hipEventDisableTiming) != hipSuccess)
                return nullptr;
        for (auto& b : c->bufs)
            if (hipHostMalloc((void**)&b, CO_META, hipHostMallocDefault) != hipSuccess) return nullptr;
        std::thread(launcher, c).detach();
        std::thread(completer, c).detach();
        g_co[device] = c;
    }
    return g_co[device];
}

int coalesced_hash(Combiner* co, const uint8_t* data, uint64_t len, uint8_t out[32]) {
    TlStage& ts = t_stage;
    if (ts.cap < len + 16) {  // this thread's pinned copy of its message
        if (ts.p) hipHostFree(ts.p);
        ts.p = nullptr;
        ts.cap = 0;
        const uint64_t want = std::max<uint64_t>(65536 + 64, len + 16);
        if (hipHostMalloc((void**)&ts.p, want, hipHostMallocDefault) != hipSuccess) return BW_ENOMEM;
        ts.cap = want;
    }
    if (len) memcpy(ts.p, data, len);
    std::shared_ptr<CoBatch> my;
    uint32_t i = 0;
    {
        std::unique_lock<std::mutex> lk(co->mu);
        for (;;) {
            if (!co->open) {
                int b = -1;
                for (int k = 0; k < CO_BUFS && b < 0; k++)
                    if (!co->buf_busy[k]) b = k;
                if (b >= 0) {
                    auto nb = std::make_shared<CoBatch>();
                    nb->buf = b;
                    nb->meta = co->bufs[b];
                    nb->ptr.reserve(256);
                    nb->len.reserve(256);
                    co->buf_busy[b] = true;
                    co->open = std::move(nb);
                }
            }
            if (co->open && co->open->n < CO_MAX_N) break;
            co->cv_room.wait(lk);  // no table free, or the open batch is full: the launcher frees one
        }
        my = co->open;
        i = my->n++;
        my->ptr.push_back((uint64_t)(uintptr_t)ts.p);
        my->len.push_back(len);
        my->maxlen = std::max(my->maxlen, len);
        my->readers.fetch_add(1, std::memory_order_relaxed);
        if (i == 0) co->cv_work.notify_one();  // a new batch: the launcher may take it now
    }
    {
        std::unique_lock<std::mutex> bl(my->mu);
        while (!my->done) my->cv.wait(bl);
    }
    const int rc = my->rc;
    if (!rc) memcpy(out, my->digp + 32ull * i, 32);
    if (my->readers.fetch_sub(1, std::memory_order_acq_rel) == 1) {  // the last reader gives the table back
        std::lock_guard<std::mutex> lk(co->mu);
        co->buf_busy[my->buf] = false;
        co->cv_room.notify_all();
    }
    return rc;
}

// ------------------------------------------------------------------ the hash service
// The default for messages of <= 64 KiB: a persistent kernel (k_b3_service, bw_b3_small.hip) whose
// workers poll a ring of request slots, one ticket each, and store each digest into a response slot
// in pinned memory over a sentinel.  With a large BAR (every MI355X host) the caller copies its
// message and writes its request straight into HBM through the BAR (fine-grained device memory;
// ~40 GB/s for a 64 KiB copy), so the GPU never reads over PCIe: a 64 KiB call went from 37 to 24 us.
// A call is a copy, a few stores and a wait on its slot: no kernel launch, no event and no library
// thread between the call and its digest (the coalescer above pays ~20 us of launch, event and
// thread hand-offs per batch before the kernel's own time).  BW_SVC_HOST_RING=1 keeps the requests
// and copies in pinned host memory.
//   * Waiting: a caller spins for SVC_SPIN_US, then sleeps on a futex of its slot; one completer
//     thread per device watches the slots of the sleeping callers and wakes each as its digest lands.
//     With more callers than cores (tokio starts one worker per core of the machine) the spinning
//     would otherwise take the cores the other callers need to post.
//   * An instance ends by itself when nothing was hashed for SVC_IDLE_US (5 ms), or after
//     SVC_LIFE_US (500 ms); a caller that finds it ended starts the next one, and a waiter without
//     its digest checks again every millisecond, which also covers a message posted just as the
//     workers gave up.  A device-wide synchronization (hipDeviceSynchronize, torch.cuda.synchronize)
//     waits for the running instance: under steady calls up to its life.  BW_SVC_LIFE_US (1,000 to
//     500,000) shortens that bound for an application that synchronizes the device while hashing;
//     50 ms cost C4 0-7 % (profiles/r05/s25_svc_stream).
//   * The stream is a non-blocking stream of the least priority (service(), below): the process's
//     other streams never queue behind the persistent kernel, and the legacy null stream does not
//     wait for it (tools/dropin_lat.cpp measures both while the service runs).
// BW_DROPIN_SERVICE=0 in the environment selects the coalescer instead (A/B).
constexpr uint32_t SVC_IDLE_US = 5000, SVC_LIFE_US = 500000;
constexpr double SVC_SPIN_US = 40;

// CPUs this process may run on at once: its affinity mask, capped by a cgroup v2 CPU quota (a
// container that lends 16 of a machine's cores shows all of them in the mask).  A caller only spins
// while fewer callers than that are waiting; past it, a spinning caller takes a core that another
// caller needs to post its message.
int usable_cpus() {
    static const int n = [] {
        cpu_set_t set;
        int c = sched_getaffinity(0, sizeof set, &set) == 0 ? CPU_COUNT(&set) : 16;
        if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char q[32] = {0};
            long period = 0;
            if (fscanf(f, "%31s %ld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
                const long quota = atol(q);
                if (quota > 0) c = std::min<int>(c, (int)std::max<long>(1, (quota + period - 1) / period));
            }
            fclose(f);
        }
        return std::max(1, c);
    }();
    return n;
}

long futex(std::atomic<uint32_t>* a, int op, uint32_t v, const timespec* ts = nullptr) {
    return syscall(SYS_futex, (uint32_t*)a, op, v, ts, nullptr, 0);
}

// The calling thread's current device for the scope, then back: the drop-ins run on the caller's
// threads (tokio workers, a torch thread), whose current device must not change under them.
struct DeviceGuard {
    int old = -1, want = 0;
    explicit DeviceGuard(int d) : want(d) {
        if (hipGetDevice(&old) != hipSuccess) old = -1;
        if (old != d) hipSetDevice(d);
    }
    ~DeviceGuard() {
        if (old >= 0 && old != want) hipSetDevice(old);
    }
};

int64_t steady_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

// A caller gives up on its ticket after SVC_WAIT_US without its slot or its digest (the GPU did not
// run the service for that long: a neighbour holding every CU, a device fault) and returns BW_EAGAIN;
// the ticket is then abandoned, never left unreturned (svc_reclaim).
constexpr double SVC_WAIT_US = 10e6;

struct Service {
    int device = 0;
    hipStream_t st = nullptr;
    B3SvcReq* req = nullptr;    // HBM through the BAR (vram), else pinned
    B3SvcResp* resp = nullptr;  // pinned
    bool vram = false;          // requests and message copies in HBM, written by the CPU (large BAR)
    B3SvcCtl* ctl = nullptr;    // pinned
    B3SvcDev* dev = nullptr;    // device
    uint32_t* proc = nullptr;   // device
    std::atomic<uint64_t> next{0};
    std::unique_ptr<std::atomic<uint64_t>[]> free_at;  // per slot: the ticket that may use it next
    std::unique_ptr<std::atomic<uint32_t>[]> sleep;    // per slot: 1 = its caller sleeps, 2 = woken
    std::atomic<uint32_t> sleepers{0};
    std::atomic<int> waiting{0};  // callers between their post and their digest
    std::atomic<uint32_t> comp_gen{0};  // the completer's futex word (bumped when a caller goes to sleep)
    std::mutex mu;
    std::atomic<uint32_t> epoch{0};  // the last instance launched
    std::atomic<uint64_t> front{0};  // tickets below it have returned to their callers (under mu)
    std::atomic<uint64_t> launches{0}, messages{0};
    // tickets whose callers gave up: ticket -> whether its request was posted.  Each is
    // handed back by svc_reclaim, so `front` and the slot's next ticket never wait for it
    std::mutex ab_mu;
    std::map<uint64_t, bool> abandoned;
    std::atomic<uint32_t> ab_pending{0};
    std::atomic<uint64_t> n_abandoned{0}, n_reclaimed{0}, n_recovered{0};
    std::atomic<int64_t> probe_at{0};  // the last stream query (at most one per millisecond)
    // message copies of threads that exited, reused by later threads (freeing device
    // memory synchronizes the device, which waits for the running instance, up to its life)
    std::mutex stage_mu;
    std::vector<uint8_t*> stage_pool;
    std::atomic<uint64_t> calls{0};
    uint64_t fault_after = UINT64_MAX;  // BW_SVC_FAULT_AFTER=n (tests): call n gives up right after posting
};

std::mutex g_svc_mu;
Service* g_svc[64] = {};
std::atomic<int> g_svc_mode{-1};  // -1 unknown, 0 coalescer, 1 service
const bool g_svc_trace = getenv("BW_SVC_TRACE") != nullptr;  // diagnostics of slow calls on stderr

bool service_enabled() {
    int m = g_svc_mode.load(std::memory_order_relaxed);
    if (m < 0) {
        const char* e = getenv("BW_DROPIN_SERVICE");
        m = (e && e[0] == '0') ? 0 : 1;
        g_svc_mode.store(m, std::memory_order_relaxed);
    }
    return m == 1;
}

uint32_t svc_dead(const Service* sv) { return __atomic_load_n(&sv->ctl->dead, __ATOMIC_ACQUIRE); }

// the slot holds ticket t's digest: no word equals its sentinel
inline bool svc_done(const B3SvcResp* sl, uint64_t t, uint64_t d[4]) {
    const uint32_t seq = (uint32_t)(t + 1);
    for (int k = 0; k < 4; k++) {
        d[k] = __atomic_load_n(&sl->digest[k], __ATOMIC_ACQUIRE);
        if (d[k] == b3svc_sentinel(seq, k)) return false;
    }
    return true;
}

// Hand the slots of abandoned tickets on.  Ticket t is reclaimed once it holds its slot (free_at ==
// t) and no worker can still write its response slot: it was never posted (its caller gave up
// waiting for the slot), its digest has landed, or no instance runs (`idle`).  Its request is marked
// cancelled first, so a worker of a later instance that reserves it moves on; then the slot goes to
// ticket t + RING and `front` may pass t.
void svc_reclaim(Service* sv, bool idle) {
    if (sv->ab_pending.load(std::memory_order_acquire) == 0) return;
    std::lock_guard<std::mutex> lk(sv->ab_mu);
    for (bool moved = true; moved;) {  // (a reclaimed slot may pass to another abandoned ticket)
        moved = false;
        for (auto it = sv->abandoned.begin(); it != sv->abandoned.end();) {
            const uint64_t t = it->first;
            const uint32_t i = (uint32_t)(t % B3_SVC_RING);
            uint64_t d[4];
            if (sv->free_at[i].load(std::memory_order_acquire) != t ||
                (it->second && !idle && !svc_done(sv->resp + i, t, d))) {
                ++it;
                continue;
            }
            __atomic_store_n(&sv->req[i].lenseq, ((uint64_t)(uint32_t)(t + 1) << 32) | B3SVC_CANCEL, __ATOMIC_RELEASE);
            _mm_sfence();  // (through the BAR: the cancel lands before the slot's next request)
            sv->free_at[i].store(t + B3_SVC_RING, std::memory_order_release);
            it = sv->abandoned.erase(it);
            sv->ab_pending.fetch_sub(1, std::memory_order_acq_rel);
            sv->n_reclaimed.fetch_add(1, std::memory_order_relaxed);
            moved = true;
        }
    }
}

void svc_abandon(Service* sv, uint64_t t, bool posted) {
    std::lock_guard<std::mutex> lk(sv->ab_mu);
    sv->abandoned.emplace(t, posted);
    sv->ab_pending.fetch_add(1, std::memory_order_acq_rel);
    sv->n_abandoned.fetch_add(1, std::memory_order_relaxed);
    if (g_svc_trace) fprintf(stderr, "[bw svc] ticket %llu abandoned (%s)\n", (unsigned long long)t, posted ? "posted" : "unposted");
}

// Start an instance unless one is running (the last launched has not published its end).  With
// `probe` (the waiting callers, every millisecond) also ask the runtime whether the instance's grid
// is still on its stream: an instance that finished without publishing its end would otherwise
// strand every posted ticket (round 5's exit count could miss workers that left before block 0 ran;
// the count is cumulative now, so this is a second line of defence, counted in n_recovered).
int svc_ensure(Service* sv, bool probe = false) {
    const uint32_t e = sv->epoch.load(std::memory_order_acquire);
    if (e != 0 && svc_dead(sv) != e) {
        if (!probe) return BW_OK;
        const int64_t now = steady_ns();
        int64_t last = sv->probe_at.load(std::memory_order_relaxed);
        if (now - last < 1000000 || !sv->probe_at.compare_exchange_strong(last, now)) return BW_OK;
        if (hipStreamQuery(sv->st) != hipSuccess) return BW_OK;  // still running
        std::lock_guard<std::mutex> lk(sv->mu);
        if (sv->epoch.load(std::memory_order_relaxed) != e || svc_dead(sv) == e) return BW_OK;
        __atomic_store_n(&sv->ctl->dead, e, __ATOMIC_RELEASE);
        sv->n_recovered.fetch_add(1, std::memory_order_relaxed);
        if (g_svc_trace) fprintf(stderr, "[bw svc] epoch %u finished without publishing its end\n", e);
    }
    std::lock_guard<std::mutex> lk(sv->mu);
    const uint32_t e2 = sv->epoch.load(std::memory_order_relaxed);
    if (e2 != 0 && svc_dead(sv) != e2) return BW_OK;
    DeviceGuard g(sv->device);
    (void)hipGetLastError();  // (clear an earlier call's error on this thread)
    svc_reclaim(sv, true);  // no instance runs: every abandoned ticket holding its slot is handed on
    // the first ticket not yet returned to its caller: the new instance reserves from there
    uint64_t lo = sv->front.load(std::memory_order_relaxed);
    const uint64_t hi = sv->next.load(std::memory_order_acquire);
    while (lo < hi && sv->free_at[lo % B3_SVC_RING].load(std::memory_order_acquire) > lo) lo++;
    sv->front.store(lo, std::memory_order_relaxed);
    static const uint32_t life = [] {  // BW_SVC_LIFE_US (see above)
        const char* e = getenv("BW_SVC_LIFE_US");
        return e && atoi(e) > 0 ? (uint32_t)std::min(std::max(atoi(e), 1000), (int)SVC_LIFE_US) : SVC_LIFE_US;
    }();
    launch_b3_service(sv->st, sv->req, sv->resp, sv->ctl, sv->dev, sv->proc, e2 + 1, (uint32_t)lo, SVC_IDLE_US, life);
    if (const hipError_t e = hipGetLastError()) {
        if (g_svc_trace) fprintf(stderr, "[bw svc] launch failed: %s\n", hipGetErrorString(e));
        return BW_EHIP;
    }
    sv->epoch.store(e2 + 1, std::memory_order_release);
    sv->launches.fetch_add(1, std::memory_order_relaxed);
    if (g_svc_trace) fprintf(stderr, "[bw svc] launched epoch %u\n", e2 + 1);
    return BW_OK;
}

// wakes the sleeping callers whose digests landed (tickets t with t % SVC_COMPLETERS == k); sleeps
// itself while no caller sleeps.  Several of them: at 256 callers one thread making every wake-up
// system call (~600 k a second) was the limit.
// A completer that found nothing to wake yields its core (round 6): with more callers than cores
// (C4 through the drop-in at 256 threads on a 16-core share) four completers polling with only a
// pause between scans held 4 of the 16 cores whenever any caller slept.  sched_yield returns at once
// when no other thread wants the core, so an idle machine still polls.  BW_SVC_COMPLETER=spin keeps
// the old loop (A/B).
constexpr int SVC_COMPLETERS = 4;
const bool g_completer_spin = [] {
    const char* e = getenv("BW_SVC_COMPLETER");
    return e && strcmp(e, "spin") == 0;
}();
void svc_completer(Service* sv, int k) {
    uint64_t lo = 0;  // tickets below lo have returned to their callers
    for (;;) {
        const uint32_t gen = sv->comp_gen.load(std::memory_order_acquire);
        if (sv->sleepers.load(std::memory_order_acquire) == 0) {
            futex(&sv->comp_gen, FUTEX_WAIT_PRIVATE, gen);
            continue;
        }
        const uint64_t hi = sv->next.load(std::memory_order_acquire);
        while (lo < hi && sv->free_at[lo % B3_SVC_RING].load(std::memory_order_acquire) > lo) lo++;
        bool woke = false;
        for (uint64_t t = lo + ((k - lo % SVC_COMPLETERS) + SVC_COMPLETERS) % SVC_COMPLETERS; t < hi; t += SVC_COMPLETERS) {
            const uint32_t i = (uint32_t)(t % B3_SVC_RING);
            uint64_t d[4];
            if (sv->sleep[i].load(std::memory_order_acquire) == 1 && svc_done(sv->resp + i, t, d)) {
                uint32_t one = 1;
                if (sv->sleep[i].compare_exchange_strong(one, 2)) {
                    futex(&sv->sleep[i], FUTEX_WAKE_PRIVATE, 1);
                    woke = true;
                }
            }
        }
        if (woke || g_completer_spin) __builtin_ia32_pause();
        else sched_yield();
    }
}

// process exit: end the running instance and wait (bounded) for its grid to drain
void svc_atexit() {
    for (int d = 0; d < 64; d++)
        if (Service* sv = g_svc[d]) {
            __atomic_store_n(&sv->ctl->stop, 1u, __ATOMIC_RELEASE);
            // (an instance ends within microseconds of the stop word, or at its life limit)
            for (int i = 0; i < 4000 && hipStreamQuery(sv->st) == hipErrorNotReady; i++) usleep(500);
        }
}

int device_count() {
    static const int n = [] {
        int c = 0;
        return hipGetDeviceCount(&c) == hipSuccess ? c : 0;
    }();
    return n;
}

bool g_svc_failed[64] = {};  // (under g_svc_mu) creation failed once: every later call goes to a context

Service* service(int device) {
    if (device < 0 || device >= 64 || device >= device_count()) return nullptr;
    std::lock_guard<std::mutex> lk(g_svc_mu);
    if (!g_svc[device] && !g_svc_failed[device]) {
        g_svc_failed[device] = true;  // (cleared below once the service is complete)
        auto* sv = new Service();  // lives as long as the process
        sv->device = device;
        DeviceGuard g(device);
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu <= 0)
            return nullptr;
        std::vector<uint32_t> mask((ncu + 31) / 32, 0xFFFFFFFFu);
        if (ncu % 32) mask.back() = (1u << (ncu % 32)) - 1;
        // The persistent kernel needs a stream that neither holds up other work nor is held up by it
        // (profiles/r05/s25_svc_stream): a plain stream shares one of the process's few hardware
        // queues (GPU_MAX_HW_QUEUES) with other streams, whose kernels then wait behind the running
        // instance (up to its 500 ms life); a CU-masked stream gets a queue of its own but is a
        // blocking stream, so every legacy-null-stream call (a bare hipMemcpy, PyTorch's default
        // stream) waits for the instance to end.  A non-blocking stream of the least priority has
        // both: the runtime keeps a queue pool per priority, and nothing else here asks for "low".
        // BW_SVC_STREAM=cumask|plain selects the other two (A/B only).
        const char* sk = getenv("BW_SVC_STREAM");
        const std::string skind = sk ? sk : "low";
        int least = 0, greatest = 0;
        if (skind == "cumask" ? hipExtStreamCreateWithCUMask(&sv->st, (uint32_t)mask.size(), mask.data()) != hipSuccess
            : skind == "plain"
                ? hipStreamCreateWithFlags(&sv->st, hipStreamNonBlocking) != hipSuccess
                : hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess ||
                      hipStreamCreateWithPriority(&sv->st, hipStreamNonBlocking, least) != hipSuccess)
            return nullptr;
        if (g_svc_trace)
            fprintf(stderr, "[svc] device %d stream %s (priority range %d..%d)\n", device, skind.c_str(), least, greatest);
        int large_bar = 0;
        hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, device);
        const char* hr = getenv("BW_SVC_HOST_RING");
        sv->vram = large_bar && !(hr && hr[0] == '1');
        if ((sv->vram ? hipExtMallocWithFlags((void**)&sv->req, sizeof(B3SvcReq) * B3_SVC_RING, hipDeviceMallocFinegrained)
                      : hipHostMalloc((void**)&sv->req, sizeof(B3SvcReq) * B3_SVC_RING, hipHostMallocDefault)) != hipSuccess ||
            hipHostMalloc((void**)&sv->resp, sizeof(B3SvcResp) * B3_SVC_RING, hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc((void**)&sv->ctl, sizeof(B3SvcCtl), hipHostMallocDefault) != hipSuccess ||
            hipMalloc((void**)&sv->dev, sizeof(B3SvcDev)) != hipSuccess ||
            hipMalloc((void**)&sv->proc, sizeof(uint32_t) * B3_SVC_RING) != hipSuccess)
            return nullptr;
        memset(sv->resp, 0, sizeof(B3SvcResp) * B3_SVC_RING);
        if (hipMemset(sv->req, 0, sizeof(B3SvcReq) * B3_SVC_RING) != hipSuccess) return nullptr;
        memset(sv->ctl, 0, sizeof(B3SvcCtl));
        if (hipMemset(sv->dev, 0, sizeof(B3SvcDev)) != hipSuccess ||
            hipMemset(sv->proc, 0, sizeof(uint32_t) * B3_SVC_RING) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
            return nullptr;
        sv->free_at.reset(new std::atomic<uint64_t>[B3_SVC_RING]);
        sv->sleep.reset(new std::atomic<uint32_t>[B3_SVC_RING]);
        for (uint32_t i = 0; i < B3_SVC_RING; i++) {
            sv->free_at[i].store(i);
            sv->sleep[i].store(0);
        }
        if (const char* f = getenv("BW_SVC_FAULT_AFTER")) sv->fault_after = strtoull(f, nullptr, 10);
        for (int k = 0; k < SVC_COMPLETERS; k++) std::thread(svc_completer, sv, k).detach();
        static std::once_flag once;
        std::call_once(once, [] { atexit(svc_atexit); });
        g_svc[device] = sv;
        g_svc_failed[device] = false;
    }
    return g_svc[device];
}

// This thread's copy area for its messages to each device's service: in that device's HBM (written
// through the BAR) or pinned, 64 KiB + 64 (every message the service takes fits, so it is never
// reallocated).  Allocated on the service's device (a tokio thread's current device is
// 0 whatever service it calls), one per (thread, device), and given back to the service's pool when
// the thread exits instead of freed (hipFree would synchronize the device).
constexpr uint64_t SVC_STAGE_BYTES = B3_MSG_MAX + 64;
struct TlVStages {
    uint8_t* p[64] = {};
    Service* sv[64] = {};
    ~TlVStages() {
        for (int d = 0; d < 64; d++)
            if (p[d]) {
                std::lock_guard<std::mutex> lk(sv[d]->stage_mu);
                sv[d]->stage_pool.push_back(p[d]);
            }
    }
};
thread_local TlVStages t_vstages;

uint8_t* svc_stage(Service* sv) {
    TlVStages& ts = t_vstages;
    const int d = sv->device;
    if (ts.p[d]) return ts.p[d];
    {
        std::lock_guard<std::mutex> lk(sv->stage_mu);
        if (!sv->stage_pool.empty()) {
            ts.p[d] = sv->stage_pool.back();
            sv->stage_pool.pop_back();
        }
    }
    if (!ts.p[d]) {
        DeviceGuard g(d);
        uint8_t* p = nullptr;
        if ((sv->vram ? hipExtMallocWithFlags((void**)&p, SVC_STAGE_BYTES, hipDeviceMallocFinegrained)
                      : hipHostMalloc((void**)&p, SVC_STAGE_BYTES, hipHostMallocDefault)) != hipSuccess)
            return nullptr;
        ts.p[d] = p;
    }
    ts.sv[d] = sv;
    return ts.p[d];
}

// One message (<= 64 KiB) through the device's service.  BW_EAGAIN when the service could not take
// it (no staging memory, no instance could be launched, or no slot / digest within SVC_WAIT_US); the
// ticket is then abandoned and reclaimed, never left taken.
int service_hash(Service* sv, const uint8_t* data, uint64_t len, uint8_t out[32]) {
    uint8_t* stage = svc_stage(sv);
    if (!stage) return BW_EAGAIN;
    if (len) memcpy(stage, data, len);
    _mm_sfence();  // (the copy reaches HBM before the request that names it: writes through the BAR are
                   // write-combined and only ordered by a fence)
    const uint64_t call = sv->calls.fetch_add(1, std::memory_order_relaxed);
    const uint64_t t = sv->next.fetch_add(1, std::memory_order_relaxed);
    const uint32_t i = (uint32_t)(t % B3_SVC_RING), seq = (uint32_t)(t + 1);
    const auto t0 = std::chrono::steady_clock::now();
    auto us_now = [&] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); };
    // the slot is free once its previous ticket returned or was reclaimed (a full ring: 4,096 calls
    // in flight)
    for (uint32_t it = 0; sv->free_at[i].load(std::memory_order_acquire) != t; it++) {
        std::this_thread::yield();
        if ((it & 255) != 255) continue;
        svc_reclaim(sv, false);  // the slot's holder may be an abandoned ticket whose digest landed
        if (svc_ensure(sv, true) != BW_OK || us_now() > SVC_WAIT_US) {
            std::lock_guard<std::mutex> lk(sv->ab_mu);
            if (sv->free_at[i].load(std::memory_order_acquire) == t) break;  // handed over just now
            sv->abandoned.emplace(t, false);
            sv->ab_pending.fetch_add(1, std::memory_order_acq_rel);
            sv->n_abandoned.fetch_add(1, std::memory_order_relaxed);
            return BW_EAGAIN;
        }
    }
    B3SvcResp* sl = sv->resp + i;
    B3SvcReq* rq = sv->req + i;
    for (int k = 0; k < 4; k++) __atomic_store_n(&sl->digest[k], b3svc_sentinel(seq, k), __ATOMIC_RELAXED);
    __atomic_store_n(&rq->ptr, (uint64_t)(uintptr_t)stage, __ATOMIC_RELAXED);
    _mm_sfence();
    __atomic_store_n(&rq->lenseq, len | ((uint64_t)seq << 32), __ATOMIC_RELEASE);
    _mm_sfence();
    int rc = svc_ensure(sv);
    if (call == sv->fault_after) rc = BW_EAGAIN;  // (tests: give up right after posting)
    uint64_t d[4];
    if (rc == BW_OK && !svc_done(sl, t, d)) {
        bool ok = false;
        const bool spin = sv->waiting.fetch_add(1, std::memory_order_acq_rel) < usable_cpus();
        for (uint32_t it = 0; spin && !ok; it++) {
            __builtin_ia32_pause();
            if (svc_done(sl, t, d)) ok = true;
            else if ((it & 63) == 63 && us_now() > SVC_SPIN_US) break;
        }
        if (!ok) {  // sleep until the completer wakes this slot; re-check the instance every millisecond
            sv->sleep[i].store(1, std::memory_order_release);
            // the completers sleep only after seeing no sleeper, so only the first sleeper wakes them
            // (a completer that saw sleepers == 0 waits on the generation read before; this bump
            // changes it)
            if (sv->sleepers.fetch_add(1, std::memory_order_acq_rel) == 0 || g_completer_spin) {
                sv->comp_gen.fetch_add(1, std::memory_order_acq_rel);
                futex(&sv->comp_gen, FUTEX_WAKE_PRIVATE, SVC_COMPLETERS);
            }
            double next_trace = 2000;
            while (!svc_done(sl, t, d)) {
                const timespec ts1 = {0, 1000000};
                if (sv->sleep[i].load(std::memory_order_acquire) == 1) futex(&sv->sleep[i], FUTEX_WAIT_PRIVATE, 1, &ts1);
                if (svc_done(sl, t, d)) break;
                sv->sleep[i].store(1, std::memory_order_release);  // (woken early, or a timeout)
                const double us = us_now();
                if ((rc = svc_ensure(sv, true)) != BW_OK) break;
                if (g_svc_trace && us > next_trace) {
                    fprintf(stderr, "[bw svc] ticket %llu waiting %.0f us: epoch %u dead %u\n", (unsigned long long)t, us,
                            sv->epoch.load(), svc_dead(sv));
                    next_trace = us * 2;
                }
                if (us > SVC_WAIT_US) {  // the device is not running the service
                    rc = BW_EAGAIN;
                    break;
                }
            }
            sv->sleep[i].store(0, std::memory_order_release);
            sv->sleepers.fetch_sub(1, std::memory_order_acq_rel);
        }
        sv->waiting.fetch_sub(1, std::memory_order_acq_rel);
    }
    sv->messages.fetch_add(1, std::memory_order_relaxed);
    if (rc != BW_OK) {  // never left taken: a late digest may still land, so svc_reclaim waits for it
        svc_abandon(sv, t, true);
        return BW_EAGAIN;
    }
    memcpy(out, d, 32);
    sv->free_at[i].store(t + B3_SVC_RING, std::memory_order_release);
    return BW_OK;
}

// A message through the device's small-message path (the service, or the coalescer under
// BW_DROPIN_SERVICE=0) without any context: BW_EAGAIN when that path cannot take it (over 64 KiB,
// unavailable, or gave up), so the caller retries through a context it holds.
int small_call(int device, const uint8_t* data, uint64_t len, uint8_t out[32]) {
    if (len > CO_MAX_MSG) return BW_EAGAIN;
    if (service_enabled()) {
        Service* sv = service(device);
        return sv ? service_hash(sv, data, len, out) : BW_EAGAIN;
    }
    Combiner* co = device < device_count() ? combiner(device) : nullptr;
    return co ? coalesced_hash(co, data, len, out) : BW_EAGAIN;
}

// The caller holds `c`: what the small-message path cannot take runs on c's own launch path.
int hash_one(bw_ctx* c, const uint8_t* data, uint64_t len, uint8_t out[32]) {
    const int rc = small_call(ctx_device(c), data, len, out);
    if (rc != BW_EAGAIN) return rc;
    const uint64_t off = 0;
    static const uint8_t empty[16] = {0};
    return bw_blake3_hash_many(c, len ? data : empty, len, &off, &len, 1, out);
}

}  // namespace

extern "C" int bw_fastcdc_chunks_hashed(bw_ctx* c, const uint8_t* src, uint64_t len, uint32_t mn, uint32_t av,
                                        uint32_t mx, bw_chunk* out, uint64_t cap, uint64_t* n_out, uint64_t* handle) {
    if (!c || !n_out || !handle || (len && !src)) return BW_EINVAL;
    *handle = 0;
    *n_out = 0;
    // FastCDC::with_level's asserts hold for an empty source too
    if (mn < BW_MINIMUM_MIN || mn > BW_MINIMUM_MAX || av < BW_AVERAGE_MIN || av > BW_AVERAGE_MAX ||
        mx < BW_MAXIMUM_MIN || mx > BW_MAXIMUM_MAX)
        return BW_EINVAL;
    if (len == 0) return BW_OK;
    bw_params p;
    p.min_size = mn;
    p.avg_size = av;
    p.max_size = mx;
    p.flags = BW_F_NO_DEDUP;  // chunk + hash; the gate stays the caller's (add_blob)
    p.small_file_threshold = 0;
    const uint64_t off = 0;
    Masks mk;  // (avg > max passes the asserts above: bw_process_files refuses it below, with its message)
    std::vector<bw_blob> tmp(make_masks(mn, av, mx, &mk) ? 0 : chunk_bound(mk, len));
    uint64_t n = 0;
    // the file goes up as one pageable hipMemcpy, not through the context's pinned staging ring: the
    // reference's tasks call this from many threads at once (one mmap'd file each), and 16 callers
    // each fanning their memcpy out over 16 ring threads ran at 35 GB/s on C1 against 47-56 for
    // the runtime's own pageable copies (profiles/r04/s05_keptab).  BW_DROPIN_REGISTER_MIB=m (A/B,
    // VERDICT r5 #6): files of at least m MiB are page-locked in place for the copy instead
    // (hipHostRegister, read-only: the reference's mmap is a read-only mapping), so the runtime DMAs
    // them directly, then unregistered.
    static const uint64_t reg_min = [] {
        const char* e = getenv("BW_DROPIN_REGISTER_MIB");
        return e && atoll(e) > 0 ? (uint64_t)atoll(e) << 20 : UINT64_MAX;
    }();
    void* reg = nullptr;
    if (len >= reg_min) {
        const uintptr_t a = (uintptr_t)src & ~(uintptr_t)4095, b = ((uintptr_t)src + len + 4095) & ~(uintptr_t)4095;
        if (hipHostRegister((void*)a, b - a, hipHostRegisterDefault | hipHostRegisterReadOnly) == hipSuccess) reg = (void*)a;
        else (void)hipGetLastError();  // (not registrable: the pageable copy below)
    }
    const int prc = bw_process_files(c, src, len, &off, &len, 1, &p, tmp.data(), tmp.size(), &n);
    if (reg) hipHostUnregister(reg);
    if (prc) return prc;
    *n_out = n;
    if (n > cap) return BW_ENOSPC;
    auto k = std::make_shared<Kept>();
    k->base = src;
    k->len = len;
    k->off.resize(n);
    k->clen.resize(n);
    k->dig.resize(32 * n);
    for (uint64_t i = 0; i < n; i++) {
        out[i].hash = tmp[i].gear_hash;
        out[i].offset = tmp[i].offset;
        out[i].length = tmp[i].length;
        k->off[i] = tmp[i].offset;
        k->clen[i] = tmp[i].length;
        memcpy(k->dig.data() + 32 * i, tmp[i].digest, 32);
    }
    k->handle = g_kept_next++;
    {
        std::unique_lock<std::shared_mutex> lk(g_kept_mu);
        g_kept_by_base[(uintptr_t)src].push_back(k);
        g_kept_by_handle[k->handle] = k;
        g_kept_maxlen = std::max(g_kept_maxlen, len);
    }
    t_last = k;  // this thread's next lookups are its chunks (dir_packer.rs:261-266)
    *handle = k->handle;
    return BW_OK;
}

extern "C" void bw_fastcdc_release(uint64_t handle) {
    if (!handle) return;
    std::unique_lock<std::shared_mutex> lk(g_kept_mu);
    auto h = g_kept_by_handle.find(handle);
    if (h == g_kept_by_handle.end()) return;
    std::shared_ptr<Kept> k = h->second;
    k->live.store(false, std::memory_order_release);
    g_kept_by_handle.erase(h);
    auto b = g_kept_by_base.find((uintptr_t)k->base);
    if (b != g_kept_by_base.end()) {
        auto& v = b->second;
        v.erase(std::remove(v.begin(), v.end(), k), v.end());
        if (v.empty()) g_kept_by_base.erase(b);
    }
    if (g_kept_by_handle.empty()) g_kept_maxlen = 0;  // (otherwise it stays an upper bound)
}

extern "C" uint64_t bw_blake3_kept_hits(void) { return g_kept_hits.load(); }

extern "C" int bw_blake3_coalesce_stats(int device, uint64_t* batches, uint64_t* messages) {
    if (device < 0 || device >= 64) return BW_EINVAL;
    uint64_t b = 0, m = 0;
    {
        std::lock_guard<std::mutex> lk(g_co_mu);
        if (const Combiner* co = g_co[device]) {
            b += co->batches.load();
            m += co->messages.load();
        }
    }
    {
        std::lock_guard<std::mutex> lk(g_svc_mu);
        if (const Service* sv = g_svc[device]) {
            b += sv->launches.load();
            m += sv->messages.load();
        }
    }
    if (batches) *batches = b;
    if (messages) *messages = m;
    return BW_OK;
}

extern "C" int bw_blake3_hash(bw_ctx* c, const uint8_t* data, uint64_t len, uint8_t out[32]) {
    if (!c || !out || (len && !data)) return BW_EINVAL;
    return hash_one(c, data, len, out);
}

extern "C" int bw_blake3_hash_dropin(bw_ctx* c, const uint8_t* data, uint64_t len, uint8_t out[32]) {
    if (!c || !out || (len && !data)) return BW_EINVAL;
    if (len && kept_lookup(data, len, out)) return BW_OK;
    return hash_one(c, data, len, out);
}

extern "C" int bw_blake3_hash_dropin_device(int device, const uint8_t* data, uint64_t len, uint8_t out[32]) {
    if (!out || (len && !data) || device < 0 || device >= 64) return BW_EINVAL;
    if (len && kept_lookup(data, len, out)) return BW_OK;
    return small_call(device, data, len, out);
}

extern "C" int bw_blake3_service_faults(int device, uint64_t* abandoned, uint64_t* reclaimed, uint64_t* recovered) {
    if (device < 0 || device >= 64) return BW_EINVAL;
    uint64_t a = 0, r = 0, v = 0;
    {
        std::lock_guard<std::mutex> lk(g_svc_mu);
        if (const Service* sv = g_svc[device]) {
            a = sv->n_abandoned.load();
            r = sv->n_reclaimed.load();
            v = sv->n_recovered.load();
        }
    }
    if (abandoned) *abandoned = a;
    if (reclaimed) *reclaimed = r;
    if (recovered) *recovered = v;
    return BW_OK;
}

extern "C" int bw_device_count(int* n) {
    if (!n) return BW_EINVAL;
    *n = device_count();
    return BW_OK;
}
