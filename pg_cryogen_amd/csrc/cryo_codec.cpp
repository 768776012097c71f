/*
 * cryo_codec.cpp -- host side of the C ABI declared in include/cryo_codec.h.
 *
 * Thin by design: argument checks, HIP plumbing (stream, events, buffers) and
 * kernel launches.  All codec arithmetic is in the .hip kernels.  No CPU codec
 * exists in this library: if HIP or the device is unavailable every entry
 * point fails with CRYO_E_NODEV / CRYO_E_HIP.
 */
#include "cryo_codec.h"
#include "host_stage.h"
#include "kernels.h"
#include "multi_share.h"

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <pthread.h>
#include <signal.h>
#include <thread>
#include <unordered_map>
#include <vector>

/* the largest block any entry point takes: LZ4_MAX_INPUT_SIZE (2 GiB - 32 MiB), for both methods */
static constexpr size_t kMaxBlockSize = 0x7E000000u;
static bool block_size_ok(size_t block_size) { return block_size != 0 && block_size <= kMaxBlockSize; }

/* A few host threads kept by a handle (staging copies of the K-block calls) or by the multi-GPU dispatcher (one per
 * further device).  The caller of the C ABI is a PostgreSQL backend: workers are created with every signal blocked
 * (the backend's SIGUSR1/SIGTERM/SIGINT handlers must only ever run on its own thread), they are created once and
 * joined when their owner is closed, and a worker that cannot be started just is not there: run() then executes
 * the shares on the calling thread.  Nothing here throws. */
namespace {
class WorkerPool {
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(unsigned)> *job_ = nullptr;
    unsigned n_ = 0, next_ = 0, running_ = 0;
    unsigned long gen_ = 0;
    bool stop_ = false;

    void loop()
    {
        unsigned long seen = 0;
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return stop_ || (gen_ != seen && next_ < n_); });
            if (stop_) return;
            seen = gen_;
            while (next_ < n_) {
                const unsigned i = next_++;
                running_++;
                lk.unlock();
                (*job_)(i);
                lk.lock();
                running_--;
            }
            if (running_ == 0) done_.notify_all();
        }
    }

public:
    /* cpus: where the workers may run (the GPU's NUMA node for the staging workers; nullptr: anywhere) */
    explicit WorkerPool(unsigned workers, const cpu_set_t *cpus = nullptr) noexcept
    {
        sigset_t all, old;
        sigfillset(&all);
        const bool masked = pthread_sigmask(SIG_SETMASK, &all, &old) == 0;
        for (unsigned i = 0; i < workers; i++) {
            try { th_.emplace_back([this] { loop(); }); } catch (...) { break; } /* EAGAIN, bad_alloc: fewer workers */
            if (cpus) (void)pthread_setaffinity_np(th_.back().native_handle(), sizeof *cpus, cpus);
        }
        if (masked) (void)pthread_sigmask(SIG_SETMASK, &old, nullptr);
    }
    ~WorkerPool()
    {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_.notify_all();
        for (auto &t : th_) if (t.joinable()) t.join();
    }
    unsigned workers() const { return (unsigned)th_.size(); }
    /* f(0) .. f(n-1), spread over the workers and the calling thread; returns when all have run.  f must not throw. */
    void run(unsigned n, const std::function<void(unsigned)> &f) noexcept
    {
        if (n == 0) return;
        if (th_.empty() || n == 1) { for (unsigned i = 0; i < n; i++) f(i); return; }
        std::unique_lock<std::mutex> lk(mu_);
        job_ = &f; n_ = n; next_ = 0; gen_++;
        cv_.notify_all();
        while (next_ < n_) {
            const unsigned i = next_++;
            running_++;
            lk.unlock();
            f(i);
            lk.lock();
            running_--;
        }
        done_.wait(lk, [&] { return running_ == 0; });
        job_ = nullptr; n_ = 0;
    }
};

/* C++ exceptions (bad_alloc from the small host-side vectors) never cross the C ABI */
template <class F>
int guarded(F &&f) noexcept
{
    try { return f(); } catch (const std::bad_alloc &) { return CRYO_E_NOMEM; } catch (...) { return CRYO_E_HIP; }
}
} // namespace

struct cryo_codec {
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    char err[256] = {0};
    cryo_codec_counters ctr = {};
    /* scratch for the single-block host API */
    uint8_t *d_in = nullptr, *d_out = nullptr;
    size_t in_cap = 0, out_cap = 0;
    uint64_t *d_off = nullptr;
    uint32_t *d_size = nullptr;
    int32_t *d_status = nullptr;
    /* zstd decode workspace */
    void *d_ws = nullptr;
    size_t ws_cap = 0;
    /* host-buffer batch API: grow-only device buffers and one pinned staging buffer */
    uint8_t *hb_src = nullptr, *hb_dst = nullptr, *hb_meta = nullptr;
    uint8_t *d_keytab = nullptr; /* the device-resident scan calls' copy of keys and byte-string constants (kKeyTableBytes), then
                                    the grouping's bucket table (kBucketTableBytes): kDescTablesBytes in all */
    size_t hb_src_cap = 0, hb_dst_cap = 0, hb_meta_cap = 0;
    void *pin = nullptr;
    size_t pin_cap = 0;
    /* pipelined K-block calls: two pinned input and two pinned output staging buffers, a transfer stream for the
     * device-to-host direction, events */
    void *pipe_pin[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t pipe_pin_cap[4] = {0, 0, 0, 0};
    hipStream_t xfer = nullptr;
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_k[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
    /* side streams of the zstd batch pipeline (created on first use) */
    cryo::ZstdAux aux = {};
    bool have_aux = false;
    /* options (cryo_codec_set_option) */
    cryo::Lz4DecodeOpts lz4_opts = {};
    bool lz4_side_failed = false; /* the optional side stream could not be created: not tried again */
    int zstd_path = 0;
    uint32_t enc_seg = 0;   /* CRYO_OPT_ENCODE_SEGMENT_BYTES: 0 = the byte-identical encoders */
    int enc_seg_zstd_strategy = 1; /* CRYO_OPT_ENCODE_SEGMENT_ZSTD_STRATEGY: the highest zstd strategy segment mode takes */
    size_t pipe_min_bytes = (size_t)64 << 20;
    /* NUMA: the cpus of the node this GPU hangs on (sysfs local_cpulist of its PCI function, cut to what the process may
     * use); the staging workers run there and the pinned buffers are allocated from there */
    cpu_set_t local_cpus;
    bool have_local_cpus = false;
    int numa_local = 1;     /* CRYO_OPT_NUMA_LOCAL */
    int64_t ws_keep = -1;   /* CRYO_OPT_WORKSPACE_KEEP_BYTES: -1 = keep everything between calls */
    size_t ws_max = 0;      /* CRYO_OPT_WORKSPACE_MAX_BYTES: 0 = automatic */
    /* staging-copy workers (created by the first K-block call that is large enough to want them) */
    WorkerPool *pool = nullptr;
    /* device-resident block pool (CRYO_OPT_POOL_BYTES): decoded blocks of keyed calls, first in first out */
    struct PoolSlot { uint64_t key = 0, fp = 0; uint32_t csize = 0; bool valid = false; };
    size_t pool_bytes = 0, pool_block = 0;
    uint8_t *d_pool = nullptr;
    std::vector<PoolSlot> pool_slots;
    std::unordered_map<uint64_t, uint32_t> pool_index; /* key -> slot */
    uint32_t pool_head = 0;                            /* next slot to fill */
    cryo_codec_transfer_counters xfer_ctr = {};
    /* write verification (CRYO_OPT_ENCODE_VERIFY, cryo_codec_verify_batch): decoded blocks, stream tables and statuses of
     * the verification decodes (grow-only, given back like the host-buffer staging); the per-block first-mismatch words of
     * the last verified compress; the failure the last host-buffer compress call returned */
    int verify = 0;
    int zstd_checksum = 0;  /* CRYO_OPT_ZSTD_CHECKSUM */
    uint8_t *d_vfy = nullptr;
    size_t vfy_cap = 0;
    uint32_t *vfy_first = nullptr;
    /* recompression (cryo_codec_recode_batch / _blocks): the decoded chunk, its output slots and packed area.  A buffer of its
     * own: with CRYO_OPT_ENCODE_VERIFY on, the encode of a chunk verifies into d_vfy while the chunk's decoded blocks are
     * still needed */
    uint8_t *d_rec = nullptr;
    size_t rec_cap = 0;
    bool vfy_failed = false;
    uint64_t vfy_block = 0;
    uint32_t vfy_off = 0;
};

static void pool_drop(cryo_codec *c);

namespace {

int fail(cryo_codec *c, hipError_t e, const char *what)
{
    if (c) snprintf(c->err, sizeof c->err, "%s: %s", what, hipGetErrorString(e));
    return CRYO_E_HIP;
}

#define HIP_TRY(c, call)                                                                           \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) return fail((c), e_, #call);                                         \
    } while (0)

/* One handle = one GPU, but the calling thread's current device is whatever the process last set (another
 * handle's cryo_codec_open, torch.cuda.set_device, ...).  Every entry point that allocates, launches or records
 * events makes the handle's device current for its duration and restores the caller's afterwards. */
struct DevGuard {
    int prev = -1;
    bool switched = false;
    explicit DevGuard(const cryo_codec *c)
    {
        if (!c) return;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != c->device) switched = hipSetDevice(c->device) == hipSuccess;
    }
    ~DevGuard() { if (switched && prev >= 0) (void)hipSetDevice(prev); }
};

bool method_ok(int m) { return m == CRYO_METHOD_LZ4 || m == CRYO_METHOD_ZSTD; }

int ensure(cryo_codec *c, uint8_t **p, size_t *cap, size_t need)
{
    if (*cap >= need) return CRYO_OK;
    if (*p) { HIP_TRY(c, hipFree(*p)); *p = nullptr; *cap = 0; }
    HIP_TRY(c, hipMalloc((void **)p, need));
    *cap = need;
    return CRYO_OK;
}

/* the calling thread on the GPU's node for the lifetime of the object (restored afterwards): a pinned buffer is placed
 * where the thread that allocates it runs, and a K-block call's share of the staging copies runs on the caller */
struct ScopedLocalCpus {
    cpu_set_t old;
    bool active = false;
    explicit ScopedLocalCpus(const cryo_codec *c)
    {
        if (!c || !c->have_local_cpus || !c->numa_local) return;
        if (pthread_getaffinity_np(pthread_self(), sizeof old, &old) != 0) return;
        active = pthread_setaffinity_np(pthread_self(), sizeof c->local_cpus, &c->local_cpus) == 0;
    }
    /* for a K-block call: only one that stages kMinCallBytes or more repays the move */
    static constexpr size_t kMinCallBytes = (size_t)8 << 20;
    ScopedLocalCpus(const cryo_codec *c, size_t n, size_t block_size) : ScopedLocalCpus(n * block_size >= kMinCallBytes ? c : nullptr) {}
    ~ScopedLocalCpus() { if (active) (void)pthread_setaffinity_np(pthread_self(), sizeof old, &old); }
};

int ensure_pinned(cryo_codec *c, size_t need)
{
    if (c->pin_cap >= need) return CRYO_OK;
    if (c->pin) { HIP_TRY(c, hipHostFree(c->pin)); c->pin = nullptr; c->pin_cap = 0; }
    need += need / 4; /* grow-only, with head room */
    ScopedLocalCpus numa_(c);
    hipError_t e = hipHostMalloc(&c->pin, need, hipHostMallocDefault);
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return CRYO_E_NOMEM; }
    if (e != hipSuccess) return fail(c, e, "hipHostMalloc");
    c->pin_cap = need;
    return CRYO_OK;
}

int ensure_pipe(cryo_codec *c, int which, size_t need)
{
    if (c->pipe_pin_cap[which] >= need) return CRYO_OK;
    if (c->pipe_pin[which]) { HIP_TRY(c, hipHostFree(c->pipe_pin[which])); c->pipe_pin[which] = nullptr; c->pipe_pin_cap[which] = 0; }
    need += need / 8;
    ScopedLocalCpus numa_(c);
    hipError_t e = hipHostMalloc(&c->pipe_pin[which], need, hipHostMallocDefault);
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return CRYO_E_NOMEM; }
    if (e != hipSuccess) return fail(c, e, "hipHostMalloc");
    c->pipe_pin_cap[which] = need;
    return CRYO_OK;
}

int ensure_pipe_streams(cryo_codec *c)
{
    if (c->xfer) return CRYO_OK;
    HIP_TRY(c, hipStreamCreateWithFlags(&c->xfer, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) {
        HIP_TRY(c, hipEventCreateWithFlags(&c->ev_in[i], hipEventDisableTiming));
        HIP_TRY(c, hipEventCreateWithFlags(&c->ev_k[i], hipEventDisableTiming));
        HIP_TRY(c, hipEventCreateWithFlags(&c->ev_out[i], hipEventDisableTiming));
    }
    return CRYO_OK;
}

/* host copies of a K-block call, spread over a few threads (one thread moves ~8 GB/s; the staging copies of a
 * 4096-block call were its longest part) */
struct CopyJob { void *dst; const void *src; size_t len; };
unsigned host_threads()
{
    static const unsigned v = [] {
        const char *e = getenv("CRYO_HOST_THREADS");
        unsigned t = e ? (unsigned)atoi(e) : 8u, hw = std::thread::hardware_concurrency();
        if (hw && t > hw) t = hw;
        return t < 1u ? 1u : t;
    }();
    return v;
}
void parallel_copy(cryo_codec *c, const std::vector<CopyJob> &jobs)
{
    size_t total = 0;
    for (const CopyJob &j : jobs) total += j.len;
    if (total >= (4u << 20) && !c->pool && host_threads() > 1u)
        c->pool = new (std::nothrow) WorkerPool(host_threads() - 1u, c->have_local_cpus && c->numa_local ? &c->local_cpus : nullptr);
    const unsigned T = (total < (4u << 20) || !c->pool) ? 1u : c->pool->workers() + 1u;
    if (T == 1u) { for (const CopyJob &j : jobs) memcpy(j.dst, j.src, j.len); return; }
    /* equal byte shares: share t takes the jobs (or parts of jobs) covering bytes [t, t+1) * total / T */
    const std::function<void(unsigned)> share = [&](unsigned t) {
        const size_t lo = total * t / T, hi = total * (t + 1) / T;
        size_t pos = 0;
        for (const CopyJob &j : jobs) {
            const size_t a = pos > lo ? pos : lo, b = pos + j.len < hi ? pos + j.len : hi;
            if (a < b) memcpy((uint8_t *)j.dst + (a - pos), (const uint8_t *)j.src + (a - pos), b - a);
            pos += j.len;
            if (pos >= hi) break;
        }
    };
    c->pool->run(T, share);
}

/* the most workspace a call may plan for: the option, or 70 % of the free device memory plus what the handle holds */
size_t ws_budget(cryo_codec *c)
{
    if (c->ws_max) return c->ws_max;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); return ~(size_t)0; }
    return fr / 10u * 7u + c->ws_cap;
}
/* host-buffer calls end synchronised: give back what the handle holds on the device beyond CRYO_OPT_WORKSPACE_KEEP_BYTES --
 * the kernels' workspace first (LZ4 sequence index, zstd tiles), then the staging areas of the host-buffer calls themselves
 * (n x block_size each: round 4 left those out, and a backend kept GiBs of them after one large call).  Every path that ends
 * a host-buffer call comes through here: the public wrappers and each handle's share of a cryo_multi_* call (multi_run). */
void ws_trim_after_call(cryo_codec *c)
{
    if (c->ws_keep < 0) return;
    const size_t keep = (size_t)c->ws_keep;
    const size_t hb = c->hb_src_cap + c->hb_dst_cap + c->hb_meta_cap + c->vfy_cap + c->rec_cap;
    const bool drop_ws = c->d_ws && c->ws_cap > keep;
    const bool drop_hb = hb != 0 && hb + (drop_ws ? 0 : c->ws_cap) > keep;
    if (!drop_ws && !drop_hb) return;
    DevGuard dev_(c);
    (void)hipStreamSynchronize(c->stream);
    if (c->xfer) (void)hipStreamSynchronize(c->xfer);
    if (drop_ws) {
        (void)hipFree(c->d_ws);
        c->d_ws = nullptr;
        c->ws_cap = 0;
    }
    if (drop_hb) {
        auto drop = [](uint8_t *&p, size_t &cap) { if (p) (void)hipFree(p); p = nullptr; cap = 0; };
        drop(c->hb_src, c->hb_src_cap);
        drop(c->hb_dst, c->hb_dst_cap);
        drop(c->hb_meta, c->hb_meta_cap);
        drop(c->d_vfy, c->vfy_cap);
        drop(c->d_rec, c->rec_cap);
        c->vfy_first = nullptr;
    }
}

int ensure_ws(cryo_codec *c, size_t need)
{
    if (c->ws_cap >= need) return CRYO_OK;
    if (c->d_ws) { HIP_TRY(c, hipFree(c->d_ws)); c->d_ws = nullptr; c->ws_cap = 0; }
    HIP_TRY(c, hipMalloc(&c->d_ws, need));
    c->ws_cap = need;
    return CRYO_OK;
}

/* a host-buffer entry point: the call behind the exception guard, then the handle's device memory trimmed (ws_trim_after_call) */
template <class F>
int host_call(cryo_codec *c, F &&f)
{
    return guarded([&] {
        const int rc = f();
        if (c) ws_trim_after_call(c);
        return rc;
    });
}

} // namespace

extern "C" {

const char *cryo_codec_version(void)
{
    return "cryo-codec 0.2 gfx950 (lz4 block format as liblz4 1.9.3; zstd frames as libzstd 1.4.8)";
}

} /* extern "C" */
/* the cpus of the NUMA node the handle's GPU hangs on: /sys/bus/pci/devices/<bus id>/local_cpulist, cut to what the process
 * may use.  Measured on the 2-socket bench host (profiles/r04_host_api.txt): a 4 096 x 128 KiB decompress call moved between
 * 25 and 32 GB/s from call to call with its staging threads and pinned buffers wherever the scheduler put them. */
static void discover_local_cpus(cryo_codec *c)
{
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, c->device) != hipSuccess) { (void)hipGetLastError(); return; }
    for (char *p = bus; *p; p++) if (*p >= 'A' && *p <= 'F') *p = (char)(*p - 'A' + 'a');
    char path[160];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/local_cpulist", bus);
    FILE *f = fopen(path, "r");
    if (!f) return;
    char line[1024] = {0};
    const bool got = fgets(line, sizeof line, f) != nullptr;
    fclose(f);
    if (!got) return;
    cpu_set_t allowed, want;
    if (pthread_getaffinity_np(pthread_self(), sizeof allowed, &allowed) != 0) return;
    CPU_ZERO(&want);
    int n = 0;
    for (char *p = line; *p;) { /* "64-127,192-255" */
        char *end;
        const long a = strtol(p, &end, 10);
        if (end == p) break;
        long b = a;
        if (*end == '-') { p = end + 1; b = strtol(p, &end, 10); }
        for (long k = a; k <= b && k < CPU_SETSIZE; k++)
            if (k >= 0 && CPU_ISSET((int)k, &allowed)) { CPU_SET((int)k, &want); n++; }
        p = *end == ',' ? end + 1 : end;
        if (*end != ',') break;
    }
    if (n > 0 && n < CPU_COUNT(&allowed)) { c->local_cpus = want; c->have_local_cpus = true; } /* one node only: nothing to choose */
}
extern "C" {

int cryo_codec_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return CRYO_E_NODEV;
    return n;
}

int cryo_codec_open(int device, cryo_codec **out)
{
    if (!out) return CRYO_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return CRYO_E_NODEV;
    if (device < 0 || device >= n) return CRYO_E_ARG;
    cryo_codec *c = new (std::nothrow) cryo_codec;
    if (!c) return CRYO_E_NOMEM;
    c->device = device;
    if (const char *e = cryo_tuning_env("CRYO_PIPE_MIN_MB")) c->pipe_min_bytes = (size_t)atoll(e) << 20; /* 0 = always, huge = never */
    if (const char *e = cryo_tuning_env("CRYO_LZ4_DECODE_PATH")) c->lz4_opts.path = atoi(e);             /* tuning aids: the options' */
    if (const char *e = cryo_tuning_env("CRYO_LZ4_INDEX_WALKERS")) c->lz4_opts.walkers = atoi(e);        /* initial values          */
    if (const char *e = cryo_tuning_env("CRYO_LZ4_INDEX_FORM")) c->lz4_opts.index_form = atoi(e);
    if (const char *e = cryo_tuning_env("CRYO_ZSTD_DECODE_PATH")) c->zstd_path = atoi(e);
    DevGuard dev_(c); /* the caller's current device is restored on return */
    hipError_t e = hipSuccess;
    if (!dev_.switched && dev_.prev != device) e = hipSetDevice(device); /* no current device yet, or the switch failed: report it */
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_off, sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_size, sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_status, sizeof(int32_t));
    if (e == hipSuccess) { /* what one round of the LZ4 decoder holds depends on the device's compute units (a partition has fewer) */
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->lz4_opts.cus = cus;
        else (void)hipGetLastError();
    }
    if (e != hipSuccess) {
        cryo_codec_close(c);
        return CRYO_E_HIP;
    }
    discover_local_cpus(c);
    *out = c;
    return CRYO_OK;
}

void cryo_codec_close(cryo_codec *c)
{
    if (!c) return;
    DevGuard dev_(c);
    delete c->pool;
    c->pool = nullptr;
    if (c->d_pool) { if (c->stream) (void)hipStreamSynchronize(c->stream); (void)hipFree(c->d_pool); c->d_pool = nullptr; }
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->d_in) (void)hipFree(c->d_in);
    if (c->d_out) (void)hipFree(c->d_out);
    if (c->d_off) (void)hipFree(c->d_off);
    if (c->d_size) (void)hipFree(c->d_size);
    if (c->d_status) (void)hipFree(c->d_status);
    if (c->d_ws) (void)hipFree(c->d_ws);
    if (c->hb_src) (void)hipFree(c->hb_src);
    if (c->hb_dst) (void)hipFree(c->hb_dst);
    if (c->hb_meta) (void)hipFree(c->hb_meta);
    if (c->d_keytab) (void)hipFree(c->d_keytab);
    if (c->d_vfy) (void)hipFree(c->d_vfy);
    if (c->d_rec) (void)hipFree(c->d_rec);
    if (c->pin) (void)hipHostFree(c->pin);
    for (int i = 0; i < 4; i++) if (c->pipe_pin[i]) (void)hipHostFree(c->pipe_pin[i]);
    if (c->xfer) { (void)hipStreamSynchronize(c->xfer); (void)hipStreamDestroy(c->xfer); }
    for (int i = 0; i < 2; i++) {
        if (c->ev_in[i]) (void)hipEventDestroy(c->ev_in[i]);
        if (c->ev_k[i]) (void)hipEventDestroy(c->ev_k[i]);
        if (c->ev_out[i]) (void)hipEventDestroy(c->ev_out[i]);
    }
    for (int l = 0; l < cryo::kZstdLanes; l++) {
        if (c->aux.lane[l]) { (void)hipStreamSynchronize(c->aux.lane[l]); (void)hipStreamDestroy(c->aux.lane[l]); }
        if (c->aux.side[l]) { (void)hipStreamSynchronize(c->aux.side[l]); (void)hipStreamDestroy(c->aux.side[l]); }
        if (c->aux.join[l]) (void)hipEventDestroy(c->aux.join[l]);
        if (c->aux.planned[l]) (void)hipEventDestroy(c->aux.planned[l]);
        if (c->aux.seqs_done[l]) (void)hipEventDestroy(c->aux.seqs_done[l]);
    }
    if (c->aux.fork) (void)hipEventDestroy(c->aux.fork);
    if (c->lz4_opts.side) { (void)hipStreamSynchronize(c->lz4_opts.side); (void)hipStreamDestroy(c->lz4_opts.side); }
    if (c->lz4_opts.fork) (void)hipEventDestroy(c->lz4_opts.fork);
    if (c->lz4_opts.join) (void)hipEventDestroy(c->lz4_opts.join);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *cryo_codec_last_error(const cryo_codec *c) { return c ? c->err : ""; }

int cryo_codec_trim(cryo_codec *c)
{
    if (!c) return CRYO_E_ARG;
    DevGuard dev_(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->xfer) HIP_TRY(c, hipStreamSynchronize(c->xfer));
    if (c->have_aux)
        for (int l = 0; l < cryo::kZstdLanes; l++)
            if (c->aux.lane[l]) HIP_TRY(c, hipStreamSynchronize(c->aux.lane[l]));
    if (c->have_aux)
        for (int l = 0; l < cryo::kZstdLanes; l++)
            if (c->aux.side[l]) HIP_TRY(c, hipStreamSynchronize(c->aux.side[l]));
    auto drop = [](auto *&p, size_t &cap) { if (p) (void)hipFree(p); p = nullptr; cap = 0; };
    { void *w = c->d_ws; if (w) (void)hipFree(w); c->d_ws = nullptr; c->ws_cap = 0; }
    drop(c->d_in, c->in_cap);
    drop(c->d_out, c->out_cap);
    drop(c->hb_src, c->hb_src_cap);
    drop(c->hb_dst, c->hb_dst_cap);
    drop(c->hb_meta, c->hb_meta_cap);
    drop(c->d_vfy, c->vfy_cap);
    drop(c->d_rec, c->rec_cap);
    if (c->d_keytab) { (void)hipFree(c->d_keytab); c->d_keytab = nullptr; }
    c->vfy_first = nullptr;
    if (c->pin) { (void)hipHostFree(c->pin); c->pin = nullptr; c->pin_cap = 0; }
    for (int i = 0; i < 4; i++)
        if (c->pipe_pin[i]) { (void)hipHostFree(c->pipe_pin[i]); c->pipe_pin[i] = nullptr; c->pipe_pin_cap[i] = 0; }
    return CRYO_OK;
}

int cryo_codec_set_option(cryo_codec *c, int option, int64_t value)
{
    if (!c) return CRYO_E_ARG;
    switch (option) {
    case CRYO_OPT_LZ4_DECODE_PATH:
        if (value < 0 || value > 3) return CRYO_E_ARG;
        c->lz4_opts.path = (int)value;
        return CRYO_OK;
    case CRYO_OPT_LZ4_INDEX_WALKERS:
        if (value < 0 || value > 64 || (value & (value - 1)) != 0) return CRYO_E_ARG;
        c->lz4_opts.walkers = (int)value;
        return CRYO_OK;
    case CRYO_OPT_LZ4_DECODE_WAVES:
        if (value < 0 || value > 2) return CRYO_E_ARG;
        c->lz4_opts.waves = (int)value;
        return CRYO_OK;
    case CRYO_OPT_LZ4_INDEX_FORM:
        if (value < 0 || value > 2) return CRYO_E_ARG;
        c->lz4_opts.index_form = (int)value;
        return CRYO_OK;
    case CRYO_OPT_PIPE_MIN_BYTES:
        if (value < 0) return CRYO_E_ARG;
        c->pipe_min_bytes = (size_t)value;
        return CRYO_OK;
    case CRYO_OPT_ZSTD_DECODE_PATH:
        if (value < 0 || value > 3) return CRYO_E_ARG;
        c->zstd_path = (int)value;
        return CRYO_OK;
    case CRYO_OPT_WORKSPACE_KEEP_BYTES:
        if (value < -1) return CRYO_E_ARG;
        c->ws_keep = value;
        return CRYO_OK;
    case CRYO_OPT_WORKSPACE_MAX_BYTES:
        if (value < 0) return CRYO_E_ARG;
        c->ws_max = (size_t)value;
        return CRYO_OK;
    case CRYO_OPT_NUMA_LOCAL:
        if (value != 0 && value != 1) return CRYO_E_ARG;
        c->numa_local = (int)value; /* workers already started keep their placement */
        return CRYO_OK;
    case CRYO_OPT_ENCODE_SEGMENT_BYTES:
        if (value != 0 && (value < 4096 || value > 131072 || (value & (value - 1)) != 0)) return CRYO_E_ARG;
        c->enc_seg = (uint32_t)value;
        return CRYO_OK;
    case CRYO_OPT_ENCODE_SEGMENT_ZSTD_STRATEGY:
        if (value < 1 || value > 6) return CRYO_E_ARG;
        c->enc_seg_zstd_strategy = (int)value;
        return CRYO_OK;
    case CRYO_OPT_ENCODE_VERIFY:
        if (value != 0 && value != 1) return CRYO_E_ARG;
        c->verify = (int)value;
        return CRYO_OK;
    case CRYO_OPT_ZSTD_CHECKSUM:
        if (value != 0 && value != 1) return CRYO_E_ARG;
        c->zstd_checksum = (int)value;
        return CRYO_OK;
    case CRYO_OPT_POOL_BYTES: {
        if (value < 0) return CRYO_E_ARG;
        DevGuard dev_(c);
        c->pool_bytes = (size_t)value;
        if (c->pool_bytes == 0 && c->d_pool) pool_drop(c); /* a new size takes effect at the next keyed call */
        return CRYO_OK;
    }
    default:
        return CRYO_E_ARG;
    }
}

int cryo_codec_get_option(const cryo_codec *c, int option, int64_t *value)
{
    if (!c || !value) return CRYO_E_ARG;
    switch (option) {
    case CRYO_OPT_LZ4_DECODE_PATH: *value = c->lz4_opts.path; return CRYO_OK;
    case CRYO_OPT_LZ4_INDEX_WALKERS: *value = c->lz4_opts.walkers; return CRYO_OK;
    case CRYO_OPT_LZ4_DECODE_WAVES: *value = c->lz4_opts.waves; return CRYO_OK;
    case CRYO_OPT_LZ4_INDEX_FORM: *value = c->lz4_opts.index_form; return CRYO_OK;
    case CRYO_OPT_PIPE_MIN_BYTES: *value = (int64_t)c->pipe_min_bytes; return CRYO_OK;
    case CRYO_OPT_POOL_BYTES: *value = (int64_t)c->pool_bytes; return CRYO_OK;
    case CRYO_OPT_ZSTD_DECODE_PATH: *value = c->zstd_path; return CRYO_OK;
    case CRYO_OPT_WORKSPACE_KEEP_BYTES: *value = c->ws_keep; return CRYO_OK;
    case CRYO_OPT_WORKSPACE_MAX_BYTES: *value = (int64_t)c->ws_max; return CRYO_OK;
    case CRYO_OPT_NUMA_LOCAL: *value = c->numa_local && c->have_local_cpus ? 1 : 0; return CRYO_OK;
    case CRYO_OPT_ENCODE_SEGMENT_BYTES: *value = c->enc_seg; return CRYO_OK;
    case CRYO_OPT_ENCODE_SEGMENT_ZSTD_STRATEGY: *value = c->enc_seg_zstd_strategy; return CRYO_OK;
    case CRYO_OPT_ENCODE_VERIFY: *value = c->verify; return CRYO_OK;
    case CRYO_OPT_ZSTD_CHECKSUM: *value = c->zstd_checksum; return CRYO_OK;
    default: return CRYO_E_ARG;
    }
}
void *cryo_codec_stream(cryo_codec *c) { return c ? (void *)c->stream : nullptr; }

int cryo_codec_sync(cryo_codec *c)
{
    DevGuard dev_(c);
    if (!c) return CRYO_E_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CRYO_OK;
}

size_t cryo_codec_bound(int method, size_t n)
{
    if (method == CRYO_METHOD_LZ4) {
        /* LZ4_compressBound: n + n/255 + 16, 0 above LZ4_MAX_INPUT_SIZE */
        return n > kMaxBlockSize ? 0 : n + n / 255 + 16;
    }
    if (method == CRYO_METHOD_ZSTD) {
        /* ZSTD_COMPRESSBOUND: n + n/256 + (n < 128 KiB ? (128 KiB - n) >> 11 : 0) */
        return n + (n >> 8) + (n < (128u << 10) ? ((128u << 10) - n) >> 11 : 0);
    }
    return 0;
}

/* ---- device memory plumbing ---- */
int cryo_dev_alloc(cryo_codec *c, size_t bytes, void **d_ptr)
{
    DevGuard dev_(c);
    if (!c || !d_ptr) return CRYO_E_ARG;
    *d_ptr = nullptr;
    /* +64: the kernels read compressed input in aligned 16-byte pieces (up to 15 bytes past a block's end) */
    hipError_t e = hipMalloc(d_ptr, bytes + 64);
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return CRYO_E_NOMEM; }
    if (e != hipSuccess) return fail(c, e, "hipMalloc");
    return CRYO_OK;
}
int cryo_dev_free(cryo_codec *c, void *d_ptr)
{
    DevGuard dev_(c);
    if (!c) return CRYO_E_ARG;
    if (!d_ptr) return CRYO_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipFree(d_ptr));
    return CRYO_OK;
}
int cryo_dev_upload(cryo_codec *c, void *d_dst, const void *h_src, size_t bytes)
{
    DevGuard dev_(c);
    if (!c || (bytes && (!d_dst || !h_src))) return CRYO_E_ARG;
    if (!bytes) return CRYO_OK;
    HIP_TRY(c, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CRYO_OK;
}
int cryo_dev_download(cryo_codec *c, void *h_dst, const void *d_src, size_t bytes)
{
    DevGuard dev_(c);
    if (!c || (bytes && (!h_dst || !d_src))) return CRYO_E_ARG;
    if (!bytes) return CRYO_OK;
    HIP_TRY(c, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CRYO_OK;
}
int cryo_dev_memset(cryo_codec *c, void *d_dst, int value, size_t bytes)
{
    DevGuard dev_(c);
    if (!c || (bytes && !d_dst)) return CRYO_E_ARG;
    if (!bytes) return CRYO_OK;
    HIP_TRY(c, hipMemsetAsync(d_dst, value, bytes, c->stream));
    return CRYO_OK;
}

/* ---- batch codec ---- */
static int verify_pass(cryo_codec *c, int method, const uint8_t *d_raw, uint64_t raw_stride, uint32_t B, uint64_t n,
                       const uint8_t *d_comp, const uint64_t *d_comp_off, uint64_t comp_stride, const uint32_t *d_comp_size,
                       int32_t *d_status, bool has_enc_status, uint32_t *d_first_user);

/* which encoder a compress call takes, and the workspace (c->d_ws) it asks for: segment-parallel encode for blocks of more than
 * S bytes (LZ4 up to 16 MiB; zstd with a strategy from `fast` up to the handle's CRYO_OPT_ENCODE_SEGMENT_ZSTD_STRATEGY);
 * everything else the byte-identical encoders.  Recompression plans its chunks with the same two functions. */
enum EncodePath { ENC_LZ4, ENC_ZSTD, ENC_LZ4_SEGMENTED, ENC_ZSTD_SEGMENTED };
static EncodePath encode_path(const cryo_codec *c, int method, int param, uint32_t B)
{
    const uint32_t S = c->enc_seg;
    if (S && B > S && method == CRYO_METHOD_LZ4 && B <= (16u << 20)) return ENC_LZ4_SEGMENTED;
    if (S && B > S && method == CRYO_METHOD_ZSTD && cryo::zstd_segment_supported(param, B, c->enc_seg_zstd_strategy))
        return ENC_ZSTD_SEGMENTED;
    return method == CRYO_METHOD_LZ4 ? ENC_LZ4 : ENC_ZSTD;
}
static size_t encode_workspace(const cryo_codec *c, int method, int param, uint32_t B, uint64_t n)
{
    switch (encode_path(c, method, param, B)) {
    case ENC_LZ4_SEGMENTED: return cryo::lz4_compress_segmented_workspace(n, B, c->enc_seg);
    case ENC_ZSTD_SEGMENTED: return cryo::zstd_compress_segmented_workspace(n, param, B, c->enc_seg);
    case ENC_ZSTD: return cryo::zstd_compress_workspace(n, param, B);
    default: return 0;
    }
}

int cryo_codec_compress_batch(cryo_codec *c, int method, int param, const void *d_src,
                              uint64_t src_stride, uint32_t block_size, uint64_t n_blocks,
                              void *d_dst, uint64_t dst_stride, uint32_t *d_out_size,
                              int32_t *d_status)
{
    DevGuard dev_(c);
    if (!c || !method_ok(method) || !block_size_ok(block_size)) return CRYO_E_ARG;
    if (n_blocks == 0) return CRYO_OK;
    if (!d_src || !d_dst || !d_out_size || !d_status || src_stride < block_size) return CRYO_E_ARG;
    if (dst_stride < cryo_codec_bound(method, block_size)) return CRYO_E_DSTSIZE;
    const uint32_t S = c->enc_seg;
    const EncodePath path = encode_path(c, method, param, block_size);
    /* levels whose strategy has a kernel; others: CRYO_E_UNSUPPORTED */
    if (path == ENC_ZSTD && !cryo::zstd_compress_supported(param, block_size)) return CRYO_E_UNSUPPORTED;
    if (path != ENC_LZ4) {
        int rc = ensure_ws(c, encode_workspace(c, method, param, block_size, n_blocks));
        if (rc != CRYO_OK) return rc;
    }
    switch (path) {
    case ENC_LZ4_SEGMENTED:
        HIP_TRY(c, cryo::launch_lz4_compress_segmented(c->stream, (const uint8_t *)d_src, src_stride, block_size, n_blocks,
                                                       (uint8_t *)d_dst, dst_stride, param, S, d_out_size, d_status, c->d_ws,
                                                       c->ws_cap));
        break;
    case ENC_ZSTD_SEGMENTED:
        HIP_TRY(c, cryo::launch_zstd_compress_segmented(c->stream, (const uint8_t *)d_src, src_stride, block_size, n_blocks,
                                                        (uint8_t *)d_dst, dst_stride, param, S, d_out_size, d_status, c->d_ws,
                                                        c->ws_cap, c->zstd_checksum ? 4u : 0u));
        break;
    case ENC_LZ4:
        HIP_TRY(c, cryo::launch_lz4_compress(c->stream, (const uint8_t *)d_src, src_stride, block_size,
                                             n_blocks, (uint8_t *)d_dst, dst_stride, param,
                                             d_out_size, d_status));
        break;
    case ENC_ZSTD:
        HIP_TRY(c, cryo::launch_zstd_compress(c->stream, (const uint8_t *)d_src, src_stride, block_size, n_blocks,
                                              (uint8_t *)d_dst, dst_stride, param, d_out_size, d_status, c->d_ws,
                                              c->ws_cap));
        break;
    }
    /* content checksums (CRYO_OPT_ZSTD_CHECKSUM): the frames above plus the flag and XXH64 of the input, both zstd paths */
    if (method == CRYO_METHOD_ZSTD && c->zstd_checksum)
        HIP_TRY(c, cryo::launch_zstd_checksum_append(c->stream, (const uint8_t *)d_src, src_stride, block_size, n_blocks,
                                                     (uint8_t *)d_dst, dst_stride, d_out_size, d_status));
    c->ctr.blocks_compressed += n_blocks;
    c->ctr.bytes_in += n_blocks * (uint64_t)block_size;
    c->ctr.launches++;
#ifdef CRYO_DEBUG
    /* fault injection for the tests of the failure paths (debug builds only): CRYO_VERIFY_FAULT="block:byte" flips one byte
     * of that block's encoded slot before it is verified */
    if (const char *e = cryo_tuning_env("CRYO_VERIFY_FAULT")) {
        unsigned long long fb = 0, fo = 0;
        if (c->verify && sscanf(e, "%llu:%llu", &fb, &fo) == 2 && fb < n_blocks && fo < dst_stride) {
            uint8_t v = 0;
            uint8_t *p = (uint8_t *)d_dst + fb * dst_stride + fo;
            HIP_TRY(c, hipMemcpyAsync(&v, p, 1, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            v ^= 0x5A;
            HIP_TRY(c, hipMemcpyAsync(p, &v, 1, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
    }
#endif
    if (c->verify)
        return guarded([&] {
            return verify_pass(c, method, (const uint8_t *)d_src, src_stride, block_size, n_blocks, (const uint8_t *)d_dst, nullptr,
                               dst_stride, d_out_size, d_status, true, nullptr);
        });
    return CRYO_OK;
}

/* the decode of cryo_codec_decompress_batch.  verification: the automatic routes whatever the handle's decode-path options say,
 * the zstd pipeline planned within zstd_max bytes of workspace, and the counters left alone (they count the caller's decodes) */
static int decompress_routed(cryo_codec *c, int method, const void *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                             void *d_dst, uint64_t dst_stride, uint32_t block_size, uint64_t n_blocks, int32_t *d_status,
                             bool verification, size_t zstd_max)
{
    if (method == CRYO_METHOD_LZ4) {
        cryo::Lz4DecodeOpts opts = c->lz4_opts;
        if (verification) opts.path = opts.walkers = opts.waves = opts.index_form = 0;
        const size_t need = cryo::lz4_decompress_workspace(n_blocks, block_size, opts);
        if (need != 0) {
            int rc = ensure_ws(c, need);
            if (rc != CRYO_OK) return rc;
        }
        if (!c->lz4_opts.side && !c->lz4_side_failed) {
            /* the side stream of the decoder's last round (lz4_dec2.hip): lowest priority, made once -- stream and both events or
             * none of them: a handle that cannot have them decodes on one stream (an optimisation, never an error) */
            int least = 0, greatest = 0;
            hipStream_t side = nullptr;
            hipEvent_t fork = nullptr, join = nullptr;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            if (hipStreamCreateWithPriority(&side, hipStreamNonBlocking, least) == hipSuccess &&
                hipEventCreateWithFlags(&fork, hipEventDisableTiming) == hipSuccess &&
                hipEventCreateWithFlags(&join, hipEventDisableTiming) == hipSuccess) {
                c->lz4_opts.side = side; c->lz4_opts.fork = fork; c->lz4_opts.join = join;
            } else {
                (void)hipGetLastError();
                if (join) (void)hipEventDestroy(join);
                if (fork) (void)hipEventDestroy(fork);
                if (side) (void)hipStreamDestroy(side);
                c->lz4_side_failed = true;
            }
        }
        opts.side = c->lz4_opts.side; opts.fork = c->lz4_opts.fork; opts.join = c->lz4_opts.join;
        HIP_TRY(c, cryo::launch_lz4_decompress(c->stream, (const uint8_t *)d_src, d_src_off, d_src_size,
                                               (uint8_t *)d_dst, dst_stride, block_size, n_blocks,
                                               d_status, need ? c->d_ws : nullptr, need ? c->ws_cap : 0, opts));
    } else {
        const int zpath = verification ? 0 : c->zstd_path;
        const size_t need = cryo::zstd_decompress_workspace(n_blocks, block_size, zpath, verification ? zstd_max : ws_budget(c));
        int rc = ensure_ws(c, need);
        if (rc != CRYO_OK) return rc;
        if (!c->have_aux) {
            for (int l = 0; l < cryo::kZstdLanes; l++) {
                HIP_TRY(c, hipStreamCreateWithFlags(&c->aux.lane[l], hipStreamNonBlocking));
                HIP_TRY(c, hipEventCreateWithFlags(&c->aux.join[l], hipEventDisableTiming));
                HIP_TRY(c, hipStreamCreateWithFlags(&c->aux.side[l], hipStreamNonBlocking));
                HIP_TRY(c, hipEventCreateWithFlags(&c->aux.planned[l], hipEventDisableTiming));
                HIP_TRY(c, hipEventCreateWithFlags(&c->aux.seqs_done[l], hipEventDisableTiming));
            }
            HIP_TRY(c, hipEventCreateWithFlags(&c->aux.fork, hipEventDisableTiming));
            c->have_aux = true;
        }
        HIP_TRY(c, cryo::launch_zstd_decompress(c->stream, (const uint8_t *)d_src, d_src_off, d_src_size,
                                                (uint8_t *)d_dst, dst_stride, block_size, n_blocks,
                                                d_status, c->d_ws, c->ws_cap, &c->aux, zpath));
    }
    if (!verification) {
        c->ctr.blocks_decompressed += n_blocks;
        c->ctr.bytes_out += n_blocks * (uint64_t)block_size;
    }
    c->ctr.launches++;
    return CRYO_OK;
}

int cryo_codec_decompress_batch(cryo_codec *c, int method, const void *d_src,
                                const uint64_t *d_src_off, const uint32_t *d_src_size, void *d_dst,
                                uint64_t dst_stride, uint32_t block_size, uint64_t n_blocks,
                                int32_t *d_status)
{
    DevGuard dev_(c);
    if (!c || !method_ok(method) || !block_size_ok(block_size)) return CRYO_E_ARG;
    if (n_blocks == 0) return CRYO_OK;
    if (!d_src || !d_src_off || !d_src_size || !d_dst || !d_status || dst_stride < block_size)
        return CRYO_E_ARG;
    return decompress_routed(c, method, d_src, d_src_off, d_src_size, d_dst, dst_stride, block_size, n_blocks, d_status, false, 0);
}

/* ---- the shared decode loop of write verification and the stored-block check ----
 * Decode the streams of n blocks with the automatic routes into handle workspace (c->d_vfy, or the pass's own buffer), in
 * chunks of K blocks that keep
 * the decoded blocks, the stream tables, the pass's own per-chunk arrays and the decoders' workspace within the call's budget
 * (CRYO_OPT_WORKSPACE_MAX_BYTES, else what ws_budget allows), and run the pass's kernels on each decoded chunk.
 * Streams come either from a table (d_comp_off: the caller's, who keeps the slack of cryo_dev_alloc) or from the slots of a
 * compress call (d_comp + i * comp_stride, an area of exactly n * comp_stride bytes as far as we know).  The decoders read
 * aligned 16-byte pieces, so up to 15 bytes beyond a stream's end, and before its start when it is not aligned: the last slot's
 * stream -- and the first's when the area is not 16-byte aligned -- may end at the area's bound, so those "edge" slots are
 * copied (slot bytes only: in bounds) into padded workspace and decoded from there.  Every other slot is followed by a whole
 * slot of at least 16 bytes (stride >= bound >= 16) and, in an aligned area, preceded by the area's own bytes. */
namespace {
constexpr uint64_t kNoEdge = ~0ull;
struct DecodeChunk {
    uint64_t lo = 0, K = 0;          /* blocks lo .. lo + cnt - 1 of the pass; K: blocks per chunk */
    uint32_t cnt = 0;
    uint64_t e0 = kNoEdge, e1 = kNoEdge, edge_stride = 0; /* the edge blocks of this chunk (kNoEdge: none) */
    uint8_t *fixed = nullptr;        /* the pass's bytes for the whole call */
    uint8_t *own = nullptr;          /* the pass's bytes for this chunk (K * own_per_block) */
    uint8_t *dec = nullptr;          /* block lo + k decoded at dec + k * Bp */
    uint64_t Bp = 0;
    int32_t *dec_st = nullptr;       /* its decoder status at dec_st[k] (the edge blocks': entries cnt and cnt + 1) */
    uint64_t *off = nullptr;         /* the chunk's stream table (K + 2 entries), filled by the pass's prep */
    uint32_t *sz = nullptr;
};
struct DecodePass {
    const uint8_t *d_comp = nullptr;
    const uint64_t *d_comp_off = nullptr;
    uint64_t comp_stride = 0;
    const uint32_t *d_comp_size = nullptr;
    /* the pass counts nowhere: decode_pass leaves cryo_codec_counters as it found them, whatever way it returns.  Not set by
     * write verification (its decodes count as launches of the compress call that asked for it) nor by recompression (its
     * encodes count as any compress does) */
    bool quiet = false;
    DecodePass() = default;
    /* decode from the caller's stream table */
    DecodePass(const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size, bool quiet_)
        : d_comp(d_src), d_comp_off(d_src_off), d_comp_size(d_src_size), quiet(quiet_) {}
    uint64_t fixed = 0;          /* bytes of DecodeChunk::fixed */
    uint64_t own_per_block = 0;  /* bytes per block of DecodeChunk::own */
    /* before a chunk's decodes: fill its stream table (off, sz; the edge blocks' at entries cnt, cnt + 1); none: the decoders
     * read d_comp_off + lo and d_comp_size + lo as they are (no edges then) */
    std::function<int(const DecodeChunk &)> prep;
    std::function<int(const DecodeChunk &)> run; /* the pass's kernels on the decoded chunk */
    /* where the pass lives (a grow-only buffer of the handle and its capacity); none: c->d_vfy */
    uint8_t **buf = nullptr;
    size_t *cap = nullptr;
    /* workspace (c->d_ws, shared with the decoders) the pass's own kernels want for a chunk of K blocks; it counts against the
     * budget like the decoders' */
    std::function<size_t(uint64_t K)> run_ws;
    /* bytes per block that the pass's run allocates elsewhere for a chunk (a verification inside it: its decoded copy in
     * c->d_vfy): planned for when K is chosen, not part of the pass's buffer */
    uint64_t elsewhere_per_block = 0;
};
} // namespace

static int decode_chunks(cryo_codec *c, int method, uint32_t B, uint64_t n, const DecodePass &ps)
{
    uint8_t **buf = ps.buf ? ps.buf : &c->d_vfy;
    size_t *cap = ps.cap ? ps.cap : &c->vfy_cap;
    auto al = [](uint64_t x) { return (x + 255u) & ~(uint64_t)255u; };
    const uint64_t Bp = ((uint64_t)B + 15u) & ~(uint64_t)15u; /* decoded block stride: 16-byte rows for the kernels */
    uint64_t e0 = kNoEdge, e1 = kNoEdge;
    if (!ps.d_comp_off) {
        if ((uintptr_t)ps.d_comp & 15u) e0 = 0;
        if (n - 1 != e0) e1 = n - 1;
    }
    const uint64_t E = ps.d_comp_off ? 0 : al(ps.comp_stride + 64u); /* one padded edge copy */
    auto meta = [&](uint64_t K) {
        return al((K + 2) * 4u) + al((K + 2) * 8u) + al((K + 2) * 4u) + 2 * E + (ps.own_per_block ? al(K * ps.own_per_block) : 0);
    };
    size_t budget = c->ws_max;
    if (!budget) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); fr = ~(size_t)0 / 2; }
        budget = fr / 10u * 7u + c->ws_cap + *cap;
    }
    cryo::Lz4DecodeOpts auto_opts = c->lz4_opts;
    auto_opts.path = auto_opts.walkers = auto_opts.waves = auto_opts.index_form = 0;
    uint64_t K = n < (1ull << 24) ? n : (1ull << 24);
    size_t zstd_max = 0;
    for (;;) {
        const uint64_t fixed = ps.fixed + meta(K) + K * Bp + 256u + K * ps.elsewhere_per_block;
        size_t dec_ws = 0;
        if (method == CRYO_METHOD_LZ4) dec_ws = cryo::lz4_decompress_workspace(K, B, auto_opts);
        else {
            zstd_max = budget > fixed ? budget - fixed : 0;
            dec_ws = cryo::zstd_decompress_workspace(K, B, 0, zstd_max);
        }
        if (ps.run_ws) {
            const size_t w = ps.run_ws(K);
            if (w > dec_ws) dec_ws = w;
        }
        if (fixed + dec_ws <= budget || K == 1) break;
        K = (K + 1) / 2;
    }
    if (method == CRYO_METHOD_ZSTD && K == 1 && zstd_max == 0) zstd_max = ~(size_t)0; /* one block: whatever it takes */
    int rc = ensure(c, buf, cap, ps.fixed + meta(K) + K * Bp + 256u + 64u);
    if (rc != CRYO_OK) return rc;
    DecodeChunk ch;
    uint8_t *p = *buf;
    ch.K = K; ch.Bp = Bp; ch.edge_stride = E;
    ch.fixed = p;                      p += ps.fixed;
    ch.dec_st = (int32_t *)p;          p += al((K + 2) * 4u);
    ch.off = (uint64_t *)p;            p += al((K + 2) * 8u);
    ch.sz = (uint32_t *)p;             p += al((K + 2) * 4u);
    uint8_t *edge = p;                 p += 2 * E;
    ch.own = p;                        p += ps.own_per_block ? al(K * ps.own_per_block) : 0;
    ch.dec = p;
    for (uint64_t lo = 0; lo < n; lo += K) {
        const uint32_t cnt = (uint32_t)(n - lo < K ? n - lo : K);
        const uint64_t ce0 = e0 != kNoEdge && e0 >= lo && e0 < lo + cnt ? e0 : kNoEdge;
        const uint64_t ce1 = e1 != kNoEdge && e1 >= lo && e1 < lo + cnt ? e1 : kNoEdge;
        ch.lo = lo; ch.cnt = cnt; ch.e0 = ce0; ch.e1 = ce1;
        if (ce0 != kNoEdge) HIP_TRY(c, hipMemcpyAsync(edge, ps.d_comp + ce0 * ps.comp_stride, ps.comp_stride, hipMemcpyDeviceToDevice, c->stream));
        if (ce1 != kNoEdge) HIP_TRY(c, hipMemcpyAsync(edge + E, ps.d_comp + ce1 * ps.comp_stride, ps.comp_stride, hipMemcpyDeviceToDevice, c->stream));
        if (ps.prep && (rc = ps.prep(ch)) != CRYO_OK) return rc;
        const uint64_t b_lo = lo + (ce0 != kNoEdge ? 1u : 0u), b_hi = lo + cnt - (ce1 != kNoEdge ? 1u : 0u);
        if (b_hi > b_lo) {
            const uint64_t k0 = b_lo - lo;
            const uint64_t *t_off = ps.prep ? ch.off + k0 : ps.d_comp_off + b_lo;
            const uint32_t *t_sz = ps.prep ? ch.sz + k0 : ps.d_comp_size + b_lo;
            rc = decompress_routed(c, method, ps.d_comp, t_off, t_sz, ch.dec + k0 * Bp, Bp, B, b_hi - b_lo, ch.dec_st + k0, true, zstd_max);
            if (rc != CRYO_OK) return rc;
        }
        if (ce0 != kNoEdge || ce1 != kNoEdge) {
            const uint64_t a = ce0 != kNoEdge ? ce0 : ce1;
            const uint32_t t = ce0 != kNoEdge ? cnt : cnt + 1u;       /* table entry of the first edge decoded */
            const uint64_t ne = (ce0 != kNoEdge) + (ce1 != kNoEdge);
            const uint64_t stride = ne == 2 ? (ce1 - ce0) * Bp : Bp;
            rc = decompress_routed(c, method, edge, ch.off + t, ch.sz + t, ch.dec + (a - lo) * Bp, stride, B, ne, ch.dec_st + t, true, zstd_max);
            if (rc != CRYO_OK) return rc;
        }
        if ((rc = ps.run(ch)) != CRYO_OK) return rc;
    }
    return CRYO_OK;
}

static int decode_pass(cryo_codec *c, int method, uint32_t B, uint64_t n, const DecodePass &ps)
{
    const cryo_codec_counters keep = c->ctr;
    const int rc = decode_chunks(c, method, B, n, ps);
    if (ps.quiet) c->ctr = keep;
    return rc;
}

/* ---- write verification ----
 * The shared decode loop over the compressed blocks, then the compare with the raw blocks (verify.hip) and the verdict folded
 * into d_status, chunk by chunk.  The per-block first-mismatch words are the caller's (d_first_user) or held for the whole call
 * in the pass's fixed bytes (c->vfy_first: a host-buffer call reports its failing block's). */
static int verify_pass(cryo_codec *c, int method, const uint8_t *d_raw, uint64_t raw_stride, uint32_t B, uint64_t n,
                       const uint8_t *d_comp, const uint64_t *d_comp_off, uint64_t comp_stride, const uint32_t *d_comp_size,
                       int32_t *d_status, bool has_enc_status, uint32_t *d_first_user)
{
    DecodePass ps;
    ps.d_comp = d_comp; ps.d_comp_off = d_comp_off; ps.comp_stride = comp_stride; ps.d_comp_size = d_comp_size;
    ps.fixed = d_first_user ? 0 : ((n * 4u + 255u) & ~(uint64_t)255u);
    auto first_of = [&](const DecodeChunk &ch) { return d_first_user ? d_first_user : (uint32_t *)ch.fixed; };
    ps.prep = [&](const DecodeChunk &ch) -> int {
        uint32_t *first = first_of(ch);
        c->vfy_first = d_first_user ? nullptr : first;
        HIP_TRY(c, cryo::launch_verify_prep(c->stream, ch.lo, ch.cnt, d_comp_off, comp_stride, d_comp_size, has_enc_status ? d_status : nullptr,
                                            ch.e0, ch.e1, ch.edge_stride, ch.off, ch.sz, first));
        return CRYO_OK;
    };
    ps.run = [&](const DecodeChunk &ch) -> int {
        uint32_t *first = first_of(ch);
        HIP_TRY(c, cryo::launch_verify_compare(c->stream, d_raw, raw_stride, ch.dec, ch.Bp, B, ch.lo, ch.cnt, ch.sz, ch.dec_st, ch.e0, ch.e1, first));
        HIP_TRY(c, cryo::launch_verify_fold(c->stream, ch.lo, ch.cnt, ch.sz, ch.dec_st, ch.e0, ch.e1, has_enc_status, d_status, first));
        return CRYO_OK;
    };
    return decode_pass(c, method, B, n, ps);
}

/* ---- the stored-block check ----
 * The shared decode loop over the caller's stream table, then the layout rules of every decoded block (check.hip) into
 * d_result, chunk by chunk.  Its decodes count nowhere: cryo_codec_counters are what they were before the call. */
static int check_pass(cryo_codec *c, int method, const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                      uint32_t B, uint64_t n, cryo_check_result *d_result)
{
    static_assert(sizeof(cryo_check_result) == sizeof(uint2), "cryo_check_result is the kernels' uint2 {reason, offset}");
    DecodePass ps(d_src, d_src_off, d_src_size, true);
    ps.own_per_block = 8u + 8u + 4u; /* verdict, gap, first nonzero byte */
    ps.run = [&](const DecodeChunk &ch) -> int {
        uint2 *verdict = (uint2 *)ch.own, *gap = verdict + ch.K;
        uint32_t *first = (uint32_t *)(gap + ch.K);
        HIP_TRY(c, cryo::launch_check(c->stream, ch.dec, ch.Bp, B, ch.cnt, ch.dec_st, verdict, gap, first, (uint2 *)(d_result + ch.lo)));
        return CRYO_OK;
    };
    return decode_pass(c, method, B, n, ps);
}

static bool check_block_size_ok(size_t block_size) { return block_size >= 16 && block_size % 8 == 0 && block_size <= kMaxBlockSize; }

/* ---- the tuple fetch ----
 * The shared decode loop over the caller's stream table; on every decoded chunk fetch.hip writes the records of the chunk's
 * requests, places the blocks behind the running total -- which stays in device memory from chunk to chunk -- and copies the
 * tuples out.  The pass's fixed bytes hold the side table (8 bytes per request of the whole call) and, for the host-buffer call,
 * the running total; per chunk (own) each block has its sum and base and, for the host-buffer call, a row of the chunk's staging
 * area for packed bytes (a chunk's tuples take less than K * B bytes: the OVERLAP rule).  Its decodes count nowhere. */
namespace {
struct FetchIo {
    const uint64_t *d_req_first = nullptr; /* device: n + 1 entries */
    const uint16_t *d_pos = nullptr;
    uint64_t n_req = 0;
    cryo_fetch_result *d_result = nullptr;
    /* device-resident call: the caller's buffer and total */
    uint8_t *d_dst = nullptr;
    uint64_t dst_cap = 0;
    uint64_t *d_total = nullptr;
    /* host-buffer call: the request table as the host knows it, and where records and bytes go */
    const uint64_t *h_req_first = nullptr;
    uint8_t *h_dst = nullptr;
    cryo_fetch_result *h_result = nullptr;
    uint64_t h_total = 0;
};
} // namespace

static int fetch_pass(cryo_codec *c, int method, const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                      uint32_t B, uint64_t n, FetchIo &io)
{
    static_assert(sizeof(cryo_fetch_result) == sizeof(uint4), "cryo_fetch_result is the kernels' 16-byte record");
    const bool host = io.h_req_first != nullptr;
    const uint64_t side_bytes = (io.n_req * 8u + 255u) & ~(uint64_t)255u;
    const uint64_t row = ((uint64_t)B + 15u) & ~(uint64_t)15u; /* a block's share of the chunk's staging area */
    DecodePass ps(d_src, d_src_off, d_src_size, true);
    ps.fixed = side_bytes + 256u;                 /* side table; the running total of the host-buffer call */
    ps.own_per_block = 32u + (host ? row : 0u);   /* sum u64, K + 1 bases u64 (within 24 K bytes); staging row */
    ps.run = [&](const DecodeChunk &ch) -> int {
        uint2 *side = (uint2 *)ch.fixed;
        uint64_t *running = host ? (uint64_t *)(ch.fixed + side_bytes) : io.d_total;
        uint64_t *sum = (uint64_t *)ch.own, *base = sum + ch.K;
        uint8_t *stage = ch.own + 32u * ch.K;
        if (ch.lo == 0) HIP_TRY(c, hipMemsetAsync(running, 0, sizeof(uint64_t), c->stream));
        HIP_TRY(c, cryo::launch_fetch(c->stream, ch.dec, ch.Bp, B, ch.cnt, ch.dec_st, io.d_req_first + ch.lo, io.d_pos, io.n_req,
                                      (uint4 *)io.d_result, side, sum, base, running, host ? stage : io.d_dst,
                                      host ? ch.K * row : io.dst_cap, host, c->lz4_opts.cus));
        if (!host) return CRYO_OK;
        /* the chunk's records, then -- its total known from the last of them -- its bytes: two waits per chunk */
        const uint64_t r0 = io.h_req_first[ch.lo], r1 = io.h_req_first[ch.lo + ch.cnt];
        if (r1 == r0) return CRYO_OK; /* no request, no tuple */
        HIP_TRY(c, hipMemcpyAsync(io.h_result + r0, io.d_result + r0, (r1 - r0) * sizeof(cryo_fetch_result), hipMemcpyDeviceToHost,
                                  c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->xfer_ctr.d2h_bytes += (r1 - r0) * sizeof(cryo_fetch_result);
        const cryo_fetch_result &last = io.h_result[r1 - 1];
        const uint64_t end = last.off + (((uint64_t)last.len + 7u) & ~(uint64_t)7u);
        if (end < io.h_total || end - io.h_total > ch.K * row) return CRYO_E_HIP; /* not a placement */
        const uint64_t tot = end - io.h_total;
        if (end > io.dst_cap) return CRYO_E_DSTSIZE;
        if (tot) {
            HIP_TRY(c, hipMemcpyAsync(io.h_dst + io.h_total, stage, tot, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            c->xfer_ctr.d2h_bytes += tot;
        }
        io.h_total = end;
        return CRYO_OK;
    };
    return decode_pass(c, method, B, n, ps);
}

/* ---- the scan filter ----
 * The shared decode loop over the caller's stream table; on every decoded chunk filter.hip tests the keys on every tuple, places
 * the blocks behind the two running totals (bytes, records) -- which stay in device memory from chunk to chunk -- and copies the
 * matches and the records out.  Per chunk (own) each block has 16 bytes per possible item of side table, its two sums and bases
 * and, for the host-buffer call, a row of the chunk's staging areas for packed bytes and for records; the pass's fixed bytes hold
 * the host-buffer call's running totals.  Its decodes count nowhere. */
using cryo::ScanDesc; /* kernels.h: what every scan call tells its kernels about the relation and the keys */

/* what the launchers of the scan calls are told about a decoded chunk (kernels.h) */
static cryo::ScanChunk scan_chunk(const cryo_codec *c, const DecodeChunk &ch, uint32_t B)
{
    return {.stream = c->stream, .d_dec = ch.dec, .dec_stride = ch.Bp, .block_size = B, .cnt = ch.cnt, .d_dec_status = ch.dec_st,
            .cus = c->lz4_opts.cus};
}

namespace {
struct FilterIo {
    ScanDesc sd;
    bool count_only = false;
    cryo_filter_block *d_blocks = nullptr;           /* device: n rows */
    uint64_t dst_cap = 0, rec_cap = 0;
    /* device-resident call: the caller's buffers and totals */
    uint8_t *d_dst = nullptr;
    cryo_filter_rec *d_rec = nullptr;
    uint64_t *d_total = nullptr;
    /* host-buffer call: where table, records and bytes go, and how far they got */
    bool host = false;
    cryo_filter_block *h_blocks = nullptr;
    cryo_filter_rec *h_rec = nullptr;
    uint8_t *h_dst = nullptr;
    uint64_t h_bytes = 0, h_recs = 0;
};
} // namespace

/* CRYO_FILTER_TRUTH's rules for the table W of a descriptor of nkeys <= 4 keys (include/cryo_codec.h): some key, some bit, no bit
 * at or above 2^nkeys, and monotone -- W[m] implies W[m | 1 << k] for every k < nkeys */
static bool truth_table_ok(uint32_t W, uint32_t nkeys)
{
    if (nkeys == 0 || W == 0 || (W >> (1u << nkeys)) != 0) return false;
    for (uint32_t m = 0; m < (1u << nkeys); m++)
        for (uint32_t k = 0; k < nkeys; k++)
            if (((W >> m) & 1u) && !((W >> (m | 1u << k)) & 1u)) return false;
    return true;
}

/* what the kernels get of a (valid) descriptor's combination of keys: the caller's table under CRYO_FILTER_TRUTH; without the
 * flag the AND table when a key needs the <true> instantiation (table_keys), which has that one verdict path, and 0 -- the
 * <false> instantiation, the code a flag-less descriptor of integer keys and null tests has always run -- otherwise */
static uint32_t scan_truth(const cryo_filter *f, bool table_keys)
{
    if (f->flags & CRYO_FILTER_TRUTH) return f->rsv;
    return table_keys ? 1u << ((1u << f->nkeys) - 1u) : 0u; /* table_keys: nkeys is 1 .. 4, or 0 with a float aggregate column
                                                               alone (the callers count that in): table 1, every tuple a match */
}

/* ---- float keys and float aggregate columns ---- */
static bool type_is_float(uint32_t type) { return type == CRYO_KEY_FLOAT4 || type == CRYO_KEY_FLOAT8; }
/* the signed integer whose order is the float order of the double of bits b (include/cryo_codec.h: "Float keys"; filter_walk.h:
 * float_map) */
static int64_t float_map_host(uint64_t b)
{
    const uint64_t mag = b & 0x7FFFFFFFFFFFFFFFull;
    if (mag > 0x7FF0000000000000ull) return INT64_MAX;
    if (mag == 0) return 0;
    return (int64_t)(b ^ ((b >> 63) ? 0x7FFFFFFFFFFFFFFFull : 0ull));
}
/* whether a (valid) descriptor needs the float kernels: keys and cols are host memory */
static bool desc_has_float(const cryo_scan_key *keys, uint32_t nkeys, const cryo_agg_col *cols, uint32_t ncols)
{
    for (uint32_t k = 0; k < nkeys; k++)
        if (type_is_float(keys[k].type) && keys[k].op >= CRYO_OP_LT && keys[k].op <= CRYO_OP_NE) return true;
    for (uint32_t j = 0; j < ncols; j++)
        if (type_is_float(cols[j].type)) return true;
    return false;
}

/* ---- pattern keys ---- */
static bool key_is_like(const cryo_scan_key &q) { return q.op == CRYO_OP_LIKE || q.op == CRYO_OP_NOT_LIKE; }
/* whether a (valid) descriptor needs the pattern kernels: keys is host memory */
static bool desc_has_like(const cryo_scan_key *keys, uint32_t nkeys)
{
    for (uint32_t k = 0; k < nkeys; k++)
        if (key_is_like(keys[k])) return true;
    return false;
}
/* the room a pattern of n bytes gets in the key table: its compiled form (like_compile) takes at most 4 n + 8 bytes -- a segment
 * of e elements costs 4 + 4 ceil(e / 2) bytes and at least e + 1 bytes of pattern, its '%' counted, the last segment e bytes,
 * and the closing word 4 */
static size_t like_room(uint32_t n) { return 4 * (size_t)n + 16; }
static constexpr uint32_t kLikeAny = 0x100u, kLikeUtf8 = 1u << 29, kLikeHead = 1u << 30, kLikeTail = 1u << 31; /* filter_walk.h's */
/* The n pattern bytes at pat compiled for walk_like (filter_walk.h) into the zeroed like_room(n) bytes at out, or -- out null --
 * only checked.  False: the pattern ends in an unescaped '\', and nothing is promised of out.  The pattern is cut at its
 * unescaped '%' into segments; a run of '%' cuts once.  An element is 16 bits: a literal byte (any byte behind '\', and any byte
 * that is not '%', '_' or '\'), or kLikeAny for '_'.  A segment is the word {element count in bits 0-15, first element in bits
 * 16-24, kLikeUtf8 (the key's CRYO_LIKE_UTF8), kLikeHead when no '%' stands before it, kLikeTail when none stands behind it}
 * and then its elements, two a word; segments have an element at least, but the pattern without any '%' is one segment of
 * head and tail even when it is empty.  A word 0 ends the program: the room is zeroed, so it is there. */
static bool like_compile(const uint8_t *pat, uint32_t n, bool utf8, uint32_t *out)
{
    uint16_t el[CRYO_KEY_BYTES_MAX];
    uint32_t ne = 0, w = 0;
    bool cut = false; /* a '%' stands before the segment being read */
    const auto flush = [&](bool tail) {
        if (out) {
            out[w] = ne | (ne ? (uint32_t)el[0] << 16 : 0u) | (utf8 ? kLikeUtf8 : 0u) | (cut ? 0u : kLikeHead) | (tail ? kLikeTail : 0u);
            for (uint32_t e = 0; e < ne; e++) out[w + 1 + (e >> 1)] |= (uint32_t)el[e] << (16 * (e & 1));
        }
        w += 1 + ((ne + 1) >> 1);
        ne = 0;
    };
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t ch = pat[i];
        if (ch == '%') {
            if (ne) flush(false);
            cut = true;
        } else if (ch == '_') el[ne++] = kLikeAny;
        else if (ch == '\\') {
            if (++i == n) return false;
            el[ne++] = pat[i];
        } else el[ne++] = ch;
    }
    if (ne || !cut) flush(true);
    return true;
}

/* the descriptor's rules (include/cryo_codec.h); atts and keys are host memory here.  *max_att: the highest key column.  In the
 * host-buffer calls keys is f->keys itself, and the address in a pattern key's value is host memory: the pattern is looked at
 * here.  In the device-resident calls keys is the library's copy of a device array and the pattern is looked at once it has
 * been read back (key_table_device) */
static bool filter_desc_ok(const cryo_filter *f, const cryo_att *atts, const cryo_scan_key *keys, uint32_t *max_att)
{
    *max_att = 0;
    if (!f || f->natts == 0 || f->natts > CRYO_FILTER_MAX_ATTS || f->nkeys > CRYO_FILTER_MAX_KEYS ||
        (f->flags & ~(CRYO_FILTER_COUNT_ONLY | CRYO_FILTER_TRUTH)) != 0 || !atts || (f->nkeys > 0 && !keys))
        return false;
    if ((f->flags & CRYO_FILTER_TRUTH) ? !truth_table_ok(f->rsv, f->nkeys) : f->rsv != 0) return false;
    for (uint32_t i = 0; i < f->natts; i++) {
        const cryo_att &a = atts[i];
        if (a.rsv != 0 || a.attlen == 0 || a.attlen < -1) return false; /* an int16 is never above 32767 */
        if (a.attalign != 1 && a.attalign != 2 && a.attalign != 4 && a.attalign != 8) return false;
        if (a.attlen == -1 && a.attalign < 4) return false;
    }
    for (uint32_t k = 0; k < f->nkeys; k++) {
        const cryo_scan_key &q = keys[k];
        const bool cmp = q.op >= CRYO_OP_LT && q.op <= CRYO_OP_NE, set = q.op == CRYO_OP_IN || q.op == CRYO_OP_NOT_IN;
        const bool like = key_is_like(q);
        if ((q.rsv != 0 && !(cmp && q.type == CRYO_KEY_BYTES) && !set && !like) || q.att == 0 || q.att > f->natts || q.op < CRYO_OP_LT ||
            q.op > CRYO_OP_NOT_LIKE)
            return false;
        if (q.att > *max_att) *max_att = q.att;
        if (q.op == CRYO_OP_ISNULL || q.op == CRYO_OP_NOTNULL) continue;
        /* a set key: rsv the members, value their address, not looked at here beyond null; the members are never looked at */
        if (set && (q.rsv == 0 || q.rsv > CRYO_KEY_SET_MAX || q.value == 0)) return false;
        if (like) { /* rsv: the pattern's length and CRYO_LIKE_UTF8; value: the pattern's address */
            const uint32_t n = q.rsv & 0xFFFFu;
            if (q.type != CRYO_KEY_BYTES || atts[q.att - 1].attlen != -1 || (q.rsv & ~(0xFFFFu | CRYO_LIKE_UTF8)) != 0 ||
                n > CRYO_KEY_BYTES_MAX || (n > 0 && q.value == 0))
                return false;
            if (keys == f->keys && !like_compile((const uint8_t *)(uintptr_t)q.value, n, false, nullptr)) return false;
            continue;
        }
        if (q.type == CRYO_KEY_BYTES && !set) { /* rsv: the constant's length; value: its address, not looked at here beyond null */
            if (atts[q.att - 1].attlen != -1 || q.rsv > CRYO_KEY_BYTES_MAX || (q.rsv > 0 && q.value == 0)) return false;
            continue;
        }
        if (type_is_float(q.type)) { /* value: the bits of a double, every pattern a constant; no lists of floats */
            const int size = q.type == CRYO_KEY_FLOAT4 ? 4 : 8;
            const cryo_att &a = atts[q.att - 1];
            if (set || a.attlen != size || a.attalign < size) return false;
            continue;
        }
        if (q.type < CRYO_KEY_INT2 || q.type > CRYO_KEY_INT8) return false;
        const int size = q.type == CRYO_KEY_INT2 ? 2 : q.type == CRYO_KEY_INT4 ? 4 : 8;
        const cryo_att &a = atts[q.att - 1];
        if (a.attlen != size || a.attalign < size) return false;
        if (set) continue; /* value is an address */
        if (size == 2 && (q.value < INT16_MIN || q.value > INT16_MAX)) return false;
        if (size == 4 && (q.value < INT32_MIN || q.value > INT32_MAX)) return false;
    }
    return true;
}

/* ---- byte-string keys: the library's own copy ----
 * A descriptor with a CRYO_KEY_BYTES key reaches the kernels as a key table: [keys 16 x nkeys][the constants in key order, each
 * zero-padded to a multiple of 8], the whole a multiple of 16 bytes, with the value of every such key rewritten to the device
 * address of its constant in the table -- 8-byte aligned there, whatever the caller's address was.  The caller's arrays are only
 * read.  A set key (CRYO_OP_IN, CRYO_OP_NOT_IN) takes the same road: its list lies among the constants as its distinct members,
 * ascending as signed 64-bit integers, in the room of the rsv members the caller named; the table's copy of the key has rsv
 * rewritten to the distinct count and value to the set's device address.  A float key (CRYO_KEY_FLOAT4, CRYO_KEY_FLOAT8) has no
 * constant behind the keys, but the table's copy of it has value rewritten to the mapped form of the double (float_map_host),
 * which the kernels compare as an integer.  A pattern key (CRYO_OP_LIKE, CRYO_OP_NOT_LIKE) travels compiled: the pattern's n
 * bytes stay with the caller, and among the constants lie like_room(n) = 4 n + 16 bytes -- a room that n alone decides, so that
 * the table's size is known before a device-resident pattern has been read back --, 8-byte aligned, holding the program of
 * like_compile and zeros behind it; the table's copy of the key has value rewritten to the program's device address and keeps
 * its rsv.  A descriptor without any of these kinds of key has no table: its keys go to the device as they are. */
static constexpr size_t kKeyConstMax = 8u * CRYO_KEY_SET_MAX; /* the most bytes one key's constant or list takes */
static_assert(kKeyConstMax >= CRYO_KEY_BYTES_MAX, "a list is the largest constant");
static constexpr size_t kKeyTableBytes = CRYO_FILTER_MAX_KEYS * (sizeof(cryo_scan_key) + kKeyConstMax);

/* the grouping's bucket table (below) lies behind the key table in the same allocation */
static constexpr size_t kBucketTableBytes = CRYO_GROUP_MAX_BY * (sizeof(cryo_bucket) + 8u * CRYO_BUCKET_BOUNDS_MAX);
static constexpr size_t kDescTablesBytes = kKeyTableBytes + kBucketTableBytes;
static_assert(kKeyTableBytes % 16 == 0 && kBucketTableBytes % 16 == 0, "both tables are 16-byte aligned");

static bool key_is_bytes(const cryo_scan_key &q) { return q.type == CRYO_KEY_BYTES && q.op >= CRYO_OP_LT && q.op <= CRYO_OP_NE; }
static bool key_is_set(const cryo_scan_key &q) { return q.op == CRYO_OP_IN || q.op == CRYO_OP_NOT_IN; }
static bool key_is_float(const cryo_scan_key &q) { return type_is_float(q.type) && q.op >= CRYO_OP_LT && q.op <= CRYO_OP_NE; }
/* the bytes at a (valid) key's address: a byte-string constant's, a list's, a pattern's; 0: the key has none */
static size_t key_raw_len(const cryo_scan_key &q)
{
    return key_is_set(q) ? (size_t)q.rsv * 8 : key_is_bytes(q) ? (size_t)q.rsv : key_is_like(q) ? (size_t)(q.rsv & 0xFFFFu) : 0;
}
/* the bytes a (valid) key takes among the table's constants, before they are rounded up to 8: what lies at its address, but a
 * pattern's room */
static size_t key_const_len(const cryo_scan_key &q) { return key_is_like(q) ? like_room(q.rsv & 0xFFFFu) : key_raw_len(q); }

/* the bytes the constants take behind the keys of a (valid) descriptor, a multiple of 16; *any: some key needs the table */
static size_t key_consts_bytes(const cryo_scan_key *keys, uint32_t nkeys, bool *any)
{
    size_t b = 0;
    *any = false;
    for (uint32_t k = 0; k < nkeys; k++)
        if (key_is_bytes(keys[k]) || key_is_set(keys[k]) || key_is_like(keys[k])) { *any = true; b += (key_const_len(keys[k]) + 7) & ~(size_t)7; }
        else if (key_is_float(keys[k])) *any = true;
    return (b + 15) & ~(size_t)15;
}

/* the key table of a (valid) descriptor at tab (zeroed, nkeys * 16 + key_consts_bytes bytes), which will lie at device address
 * d_tab; consts[k]: where the host finds the constant of key k.  A pattern key's room holds, from its first byte on, 32-bit
 * words: per segment of the pattern {ne | first element << 16 | kLikeUtf8 | kLikeHead | kLikeTail} and ceil(ne / 2) words of two
 * 16-bit elements each (a literal byte, or kLikeAny), the low half first; then a word 0, and zeros to the room's end
 * (like_compile).  False: a pattern ends in an unescaped '\' -- the device-resident calls learn it here */
static bool key_table_fill(uint8_t *tab, uint64_t d_tab, const cryo_scan_key *keys, uint32_t nkeys, const void *const *consts)
{
    size_t at = (size_t)nkeys * sizeof(cryo_scan_key);
    for (uint32_t k = 0; k < nkeys; k++) {
        cryo_scan_key q = keys[k];
        if (key_is_set(q)) { /* at is a multiple of 8: the table is 8-byte aligned wherever it is built */
            int64_t *m = reinterpret_cast<int64_t *>(tab + at);
            memcpy(m, consts[k], (size_t)q.rsv * 8);
            std::sort(m, m + q.rsv);
            const uint32_t distinct = (uint32_t)(std::unique(m, m + q.rsv) - m);
            memset(m + distinct, 0, (size_t)(q.rsv - distinct) * 8);
            q.value = (int64_t)(d_tab + at);
            at += (size_t)q.rsv * 8;
            q.rsv = distinct;
        } else if (key_is_bytes(q)) {
            if (q.rsv) memcpy(tab + at, consts[k], q.rsv);
            q.value = (int64_t)(d_tab + at);
            at += ((size_t)q.rsv + 7) & ~(size_t)7;
        } else if (key_is_like(q)) { /* at is a multiple of 8, and so is the room rounded up */
            const uint32_t n = q.rsv & 0xFFFFu;
            if (!like_compile((const uint8_t *)consts[k], n, (q.rsv & CRYO_LIKE_UTF8) != 0, reinterpret_cast<uint32_t *>(tab + at))) return false;
            q.value = (int64_t)(d_tab + at);
            at += (like_room(n) + 7) & ~(size_t)7;
        } else if (key_is_float(q))
            q.value = float_map_host((uint64_t)q.value);
        memcpy(tab + (size_t)k * sizeof(cryo_scan_key), &q, sizeof q);
    }
    return true;
}

/* the device-resident calls: keys (host copy, validated) name constants and lists in DEVICE memory.  Reads them back together (at
 * most 4 x 8 192 bytes, one wait), builds the table in handle-owned device memory and gives its address; one more wait on the
 * stream.  Without a byte-string key or a set key: *d_keys stays the caller's array and nothing is queued. */
static int key_table_device(cryo_codec *c, const cryo_scan_key *keys, uint32_t nkeys, const void **d_keys, bool *table_keys)
{
    const size_t cb = key_consts_bytes(keys, nkeys, table_keys);
    if (!*table_keys) return CRYO_OK;
    std::vector<uint8_t> consts(CRYO_FILTER_MAX_KEYS * kKeyConstMax), tab((size_t)nkeys * sizeof(cryo_scan_key) + cb, 0);
    const void *where[CRYO_FILTER_MAX_KEYS] = {nullptr, nullptr, nullptr, nullptr};
    for (uint32_t k = 0; k < nkeys; k++) {
        const size_t len = key_raw_len(keys[k]);
        if (len == 0) continue;
        where[k] = consts.data() + (size_t)k * kKeyConstMax;
        HIP_TRY(c, hipMemcpyAsync((void *)where[k], (const void *)(uintptr_t)keys[k].value, len, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!c->d_keytab) HIP_TRY(c, hipMalloc(&c->d_keytab, kDescTablesBytes));
    if (!key_table_fill(tab.data(), (uint64_t)(uintptr_t)c->d_keytab, keys, nkeys, where)) return CRYO_E_ARG;
    HIP_TRY(c, hipMemcpyAsync(c->d_keytab, tab.data(), tab.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); /* tab is the call's own: gone when it returns */
    *d_keys = c->d_keytab;
    return CRYO_OK;
}

/* the host-buffer calls: the table into the pinned copy of the descriptor at pin_keys, which the upload puts at d_keys.  False:
 * a pattern does not compile (filter_desc_ok refuses it first when it is handed f->keys; a caller that was not is told here,
 * and uploads nothing) */
static bool key_table_host(uint8_t *pin_keys, const uint8_t *d_keys, const cryo_filter *f)
{
    bool any = false;
    (void)key_consts_bytes(f->keys, f->nkeys, &any);
    if (!any) {
        if (f->nkeys) memcpy(pin_keys, f->keys, (size_t)f->nkeys * sizeof(cryo_scan_key));
        return true;
    }
    const void *where[CRYO_FILTER_MAX_KEYS] = {nullptr, nullptr, nullptr, nullptr};
    for (uint32_t k = 0; k < f->nkeys; k++) where[k] = (const void *)(uintptr_t)f->keys[k].value;
    return key_table_fill(pin_keys, (uint64_t)(uintptr_t)d_keys, f->keys, f->nkeys, where);
}

static int filter_pass(cryo_codec *c, int method, const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                       uint32_t B, uint64_t n, FilterIo &io)
{
    static_assert(sizeof(cryo_filter_block) == 2 * sizeof(uint4) && sizeof(cryo_filter_rec) == sizeof(uint2) &&
                      sizeof(cryo_att) == 4 && sizeof(cryo_scan_key) == 16,
                  "the filter's records are the kernels'");
    const bool host = io.host, stage = host && !io.count_only;
    const uint64_t S = cryo::filter_side_stride(B);
    const uint64_t row = ((uint64_t)B + 15u) & ~(uint64_t)15u; /* a block's share of the chunk's staging area for bytes */
    DecodePass ps(d_src, d_src_off, d_src_size, true);
    ps.fixed = 256u;                                                /* the running totals of the host-buffer call */
    ps.own_per_block = 16u * S + 48u + (stage ? row + 8u * S : 0u); /* side; 2 sums, 2 x (K + 1) bases (u64); staging rows */
    ps.run = [&](const DecodeChunk &ch) -> int {
        uint64_t *running = host ? (uint64_t *)ch.fixed : io.d_total;
        uint4 *side = (uint4 *)ch.own;
        uint64_t *sum = (uint64_t *)(ch.own + 16u * S * ch.K), *base = sum + 2u * ch.K;
        uint8_t *st_dst = ch.own + (16u * S + 48u) * ch.K;
        cryo_filter_rec *st_rec = (cryo_filter_rec *)(st_dst + row * ch.K);
        if (ch.lo == 0) HIP_TRY(c, hipMemsetAsync(running, 0, 2 * sizeof(uint64_t), c->stream));
        HIP_TRY(c, cryo::launch_filter(scan_chunk(c, ch, B), io.sd,
                                       {.count_only = io.count_only, .d_blocks = (uint4 *)(io.d_blocks + ch.lo), .d_side = side, .d_sum = sum,
                                        .d_base = base, .d_running = running, .d_dst = stage ? st_dst : io.d_dst,
                                        .dst_cap = stage ? ch.K * row : io.dst_cap, .d_rec = stage ? (uint2 *)st_rec : (uint2 *)io.d_rec,
                                        .rec_cap = stage ? ch.K * S : io.rec_cap, .chunk_relative = host}));
        if (!host) return CRYO_OK;
        /* the chunk's rows of the table; then -- their number known from the rows -- its records; then -- their total known from
         * the last row and the last block's records -- its bytes */
        cryo_filter_block *rows = io.h_blocks + ch.lo;
        HIP_TRY(c, hipMemcpyAsync(rows, io.d_blocks + ch.lo, ch.cnt * sizeof(cryo_filter_block), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->xfer_ctr.d2h_bytes += ch.cnt * sizeof(cryo_filter_block);
        if (io.count_only) return CRYO_OK;
        const cryo_filter_block &last = rows[ch.cnt - 1];
        const uint64_t last_recs = (uint64_t)last.n_match + last.n_bad;
        if (rows[0].rec_first != io.h_recs || rows[0].off != io.h_bytes || last.rec_first < io.h_recs || last.off < io.h_bytes ||
            last_recs > S || last.rec_first + last_recs - io.h_recs > ch.K * S)
            return CRYO_E_HIP; /* not a placement */
        const uint64_t rec_end = last.rec_first + last_recs, nrec = rec_end - io.h_recs;
        if (rec_end > io.rec_cap) return CRYO_E_DSTSIZE;
        if (nrec) {
            HIP_TRY(c, hipMemcpyAsync(io.h_rec + io.h_recs, st_rec, nrec * sizeof(cryo_filter_rec), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            c->xfer_ctr.d2h_bytes += nrec * sizeof(cryo_filter_rec);
        }
        uint64_t end = last.off;
        for (uint64_t r = last.rec_first; r < rec_end; r++)
            if (io.h_rec[r].status == 0) end += ((uint64_t)io.h_rec[r].len + 7u) & ~(uint64_t)7u;
        if (end - io.h_bytes > ch.K * row) return CRYO_E_HIP; /* not a placement */
        const uint64_t tot = end - io.h_bytes;
        if (end > io.dst_cap) return CRYO_E_DSTSIZE;
        if (tot) {
            HIP_TRY(c, hipMemcpyAsync(io.h_dst + io.h_bytes, st_dst, tot, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            c->xfer_ctr.d2h_bytes += tot;
        }
        io.h_bytes = end;
        io.h_recs = rec_end;
        return CRYO_OK;
    };
    return decode_pass(c, method, B, n, ps);
}

/* ---- the scan aggregate ----
 * The shared decode loop over the caller's stream table; on every decoded chunk agg.hip tests the keys on every tuple and reduces
 * the aggregate columns of the matches, one row and ncols cells per block, written straight to the call's output at the chunk's
 * first block.  The pass asks for no bytes of its own, keeps no totals and waits for nothing.  Its decodes count nowhere. */
namespace {
struct AggIo {
    ScanDesc sd;
    const void *d_cols = nullptr;       /* device */
    uint32_t ncols = 0;
    cryo_agg_block *d_blocks = nullptr; /* device: n rows */
    cryo_agg_cell *d_cells = nullptr;   /* device: n * ncols cells */
};
} // namespace

/* the aggregate's descriptor rules (include/cryo_codec.h); every array is host memory here.  *max_att: the highest key or
 * aggregate column */
/* the rule of one aggregate (or group) column; raises *max_att to it.  floats: a float type is allowed (an aggregate column; a
 * group column is an integer) */
static bool agg_col_ok(const cryo_filter *f, const cryo_att *atts, const cryo_agg_col &q, uint32_t *max_att, bool floats)
{
    if (q.rsv != 0 || q.rsv2 != 0 || q.att == 0 || q.att > f->natts) return false;
    if ((q.type < CRYO_KEY_INT2 || q.type > CRYO_KEY_INT8) && !(floats && type_is_float(q.type))) return false;
    const int size = q.type == CRYO_KEY_INT2 ? 2 : (q.type == CRYO_KEY_INT4 || q.type == CRYO_KEY_FLOAT4) ? 4 : 8;
    const cryo_att &a = atts[q.att - 1];
    if (a.attlen != size || a.attalign < size) return false;
    if (q.att > *max_att) *max_att = q.att;
    return true;
}

static bool agg_desc_ok(const cryo_filter *f, const cryo_att *atts, const cryo_scan_key *keys, const cryo_agg *agg,
                        const cryo_agg_col *cols, uint32_t *max_att)
{
    if (!filter_desc_ok(f, atts, keys, max_att)) return false;
    if ((f->flags & ~CRYO_FILTER_TRUTH) != 0 || !agg || agg->ncols == 0 || agg->ncols > CRYO_AGG_MAX_COLS || agg->rsv != 0 || !cols) return false;
    for (uint32_t j = 0; j < agg->ncols; j++)
        if (!agg_col_ok(f, atts, cols[j], max_att, true)) return false;
    return true;
}

static int agg_pass(cryo_codec *c, int method, const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                    uint32_t B, uint64_t n, const AggIo &io)
{
    static_assert(sizeof(cryo_agg_block) == sizeof(uint4) && sizeof(cryo_agg_cell) == 40 && sizeof(cryo_agg_col) == 8,
                  "the aggregate's records are the kernel's");
    DecodePass ps(d_src, d_src_off, d_src_size, true);
    ps.run = [&](const DecodeChunk &ch) -> int {
        HIP_TRY(c, cryo::launch_agg(scan_chunk(c, ch, B), io.sd,
                                    {.d_cols = io.d_cols, .ncols = io.ncols, .d_blocks = (uint4 *)(io.d_blocks + ch.lo),
                                     .d_cells = io.d_cells + ch.lo * io.ncols}));
        return CRYO_OK;
    };
    return decode_pass(c, method, B, n, ps);
}

/* ---- the grouped scan ----
 * The shared decode loop over the caller's stream table; on every decoded chunk group.hip tests the keys on every tuple, groups
 * each block's matches in LDS and writes the groups to a side area, places the blocks behind the running total -- which stays in
 * device memory (*d_total) from chunk to chunk -- and copies records and cells to their places in the call's output.  Per chunk
 * (own) each block has 24 + 40 * (ncols + ntext) bytes per possible group of side area (ntext: the text group columns, whose key
 * cells lie behind a group's aggregate cells); the pass's fixed bytes hold the kernel's six column
 * slots when the caller's descriptors come as two arrays.  The pass waits for nothing.  Its decodes count nowhere. */
namespace {
struct GroupIo {
    ScanDesc sd;
    const void *d_by = nullptr, *d_cols = nullptr;   /* device: the caller's two arrays, or */
    const void *d_slots = nullptr;                   /* device: the six slots laid out already */
    uint32_t nby = 0, ncols = 0;
    cryo_group_block *d_blocks = nullptr; /* device: n rows */
    cryo_group_rec *d_groups = nullptr;   /* device: group_cap records */
    cryo_agg_cell *d_cells = nullptr;     /* device: group_cap * (ncols + ntext) cells */
    uint64_t group_cap = 0;
    uint64_t *d_total = nullptr;          /* device: the running total */
};
} // namespace

/* ---- bucketed group columns (CRYO_GROUP_BUCKETS): the library's own copy ----
 * Such a descriptor reaches the kernels (group_bucket.hip) as a bucket table: [buckets 24 x CRYO_GROUP_MAX_BY][the lists of
 * boundaries in column order], a multiple of 16 bytes.  A list lies there as its distinct boundaries, ascending as signed 64-bit
 * integers, in the room of the n the caller named; the table's copy of the bucket has n rewritten to the distinct count and value
 * to the list's device address -- 8-byte aligned there, whatever the caller's address was.  The caller's arrays are only read.
 * The device-resident call builds the table behind the key table in c->d_keytab (bucket_table_device), the host-buffer calls in
 * the descriptor's extra bytes behind the six column slots (group_blocks_impl): the pass's fixed 256 bytes hold the slots alone. */

/* where a group descriptor's buckets are: null without CRYO_GROUP_BUCKETS */
static const cryo_bucket *group_buckets(const cryo_group *grp)
{
    return grp->rsv == CRYO_GROUP_BUCKETS ? reinterpret_cast<const cryo_group_b *>(grp)->buckets : nullptr;
}

/* the rules of the nby buckets at bk (host memory); a list's address is not looked at beyond null, its members never */
static bool bucket_desc_ok(const cryo_bucket *bk, uint32_t nby)
{
    for (uint32_t j = 0; j < nby; j++) {
        const cryo_bucket &b = bk[j];
        if (b.rsv != 0 || (b.flags & ~CRYO_BUCKET_INFINITE) != 0) return false;
        if (b.kind == CRYO_BUCKET_NONE) {
            if (b.flags != 0 || b.n != 0 || b.origin != 0 || b.value != 0) return false;
        } else if (b.kind == CRYO_BUCKET_WIDTH) {
            if (b.value < 1 || b.n != 0) return false;
        } else if (b.kind == CRYO_BUCKET_BOUNDS) {
            if (b.n == 0 || b.n > CRYO_BUCKET_BOUNDS_MAX || b.value == 0 || b.origin != 0) return false;
        } else return false;
    }
    return true;
}

/* the bytes of the bucket table of nby (valid) buckets, a multiple of 16 */
static size_t bucket_table_bytes(const cryo_bucket *bk, uint32_t nby)
{
    size_t b = CRYO_GROUP_MAX_BY * sizeof(cryo_bucket);
    for (uint32_t j = 0; j < nby; j++)
        if (bk[j].kind == CRYO_BUCKET_BOUNDS) b += (size_t)bk[j].n * 8;
    return (b + 15) & ~(size_t)15;
}

/* the bucket table of nby (valid) buckets at tab (zeroed, 8-byte aligned, bucket_table_bytes bytes), which will lie at device
 * address d_tab; lists[j]: where the host finds the boundaries of bucket j */
static void bucket_table_fill(uint8_t *tab, uint64_t d_tab, const cryo_bucket *bk, uint32_t nby, const void *const *lists)
{
    size_t at = CRYO_GROUP_MAX_BY * sizeof(cryo_bucket);
    for (uint32_t j = 0; j < nby; j++) {
        cryo_bucket b = bk[j];
        if (b.kind == CRYO_BUCKET_BOUNDS) {
            int64_t *m = reinterpret_cast<int64_t *>(tab + at);
            memcpy(m, lists[j], (size_t)b.n * 8);
            std::sort(m, m + b.n);
            const uint32_t distinct = (uint32_t)(std::unique(m, m + b.n) - m);
            memset(m + distinct, 0, (size_t)(b.n - distinct) * 8);
            b.value = (int64_t)(d_tab + at);
            at += (size_t)b.n * 8;
            b.n = distinct;
        }
        memcpy(tab + (size_t)j * sizeof(cryo_bucket), &b, sizeof b);
    }
}

/* the device-resident call: bk (host copy, validated) names lists in DEVICE memory.  Reads them back together (at most 2 x 8 192
 * bytes, one wait), builds the table behind the key table in handle-owned device memory and gives its address; one more wait */
static int bucket_table_device(cryo_codec *c, const cryo_bucket *bk, uint32_t nby, const void **d_buckets)
{
    std::vector<uint64_t> lists((size_t)CRYO_GROUP_MAX_BY * CRYO_BUCKET_BOUNDS_MAX), tab(bucket_table_bytes(bk, nby) / 8, 0);
    const void *where[CRYO_GROUP_MAX_BY] = {nullptr, nullptr};
    for (uint32_t j = 0; j < nby; j++) {
        if (bk[j].kind != CRYO_BUCKET_BOUNDS) continue;
        where[j] = lists.data() + (size_t)j * CRYO_BUCKET_BOUNDS_MAX;
        HIP_TRY(c, hipMemcpyAsync((void *)where[j], (const void *)(uintptr_t)bk[j].value, (size_t)bk[j].n * 8, hipMemcpyDeviceToHost,
                                  c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!c->d_keytab) HIP_TRY(c, hipMalloc(&c->d_keytab, kDescTablesBytes));
    uint8_t *d_tab = c->d_keytab + kKeyTableBytes;
    bucket_table_fill((uint8_t *)tab.data(), (uint64_t)(uintptr_t)d_tab, bk, nby, where);
    HIP_TRY(c, hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); /* tab is the call's own: gone when it returns */
    *d_buckets = d_tab;
    return CRYO_OK;
}

/* cryo_group.rsv: nothing, buckets, or text group columns -- not both */
static bool group_rsv_ok(uint32_t rsv) { return rsv == 0 || rsv == CRYO_GROUP_BUCKETS || rsv == CRYO_GROUP_TEXT; }

/* the grouping's descriptor rules (include/cryo_codec.h); every array is host memory here -- bk: the nby buckets of a
 * CRYO_GROUP_BUCKETS descriptor, whose pointer within *grp is held against its rules here too.  *max_att: the highest key, group
 * or aggregate column; *ncols: the aggregate columns (0 with a null agg); *text: bit j set when group column j is a byte string,
 * which CRYO_GROUP_TEXT alone allows, on a varlena column */
static bool group_desc_ok(const cryo_filter *f, const cryo_att *atts, const cryo_scan_key *keys, const cryo_group *grp,
                          const cryo_agg_col *by, const cryo_bucket *bk, const cryo_agg *agg, const cryo_agg_col *cols, uint32_t *max_att,
                          uint32_t *ncols, uint32_t *text)
{
    *ncols = 0;
    *text = 0;
    if (!filter_desc_ok(f, atts, keys, max_att)) return false;
    if ((f->flags & ~CRYO_FILTER_TRUTH) != 0 || !grp || grp->nby == 0 || grp->nby > CRYO_GROUP_MAX_BY || !group_rsv_ok(grp->rsv) || !by)
        return false;
    for (uint32_t j = 0; j < grp->nby; j++) {
        const cryo_agg_col &q = by[j];
        if (grp->rsv == CRYO_GROUP_TEXT && q.type == CRYO_KEY_BYTES) {
            if (q.rsv != 0 || q.rsv2 != 0 || q.att == 0 || q.att > f->natts || atts[q.att - 1].attlen != -1) return false;
            if (q.att > *max_att) *max_att = q.att;
            *text |= 1u << j;
        } else if (!agg_col_ok(f, atts, q, max_att, false)) return false;
    }
    if (grp->rsv == CRYO_GROUP_BUCKETS &&
        (!group_buckets(grp) || ((uintptr_t)group_buckets(grp) & 7u) != 0 || !bk || !bucket_desc_ok(bk, grp->nby)))
        return false;
    if (!agg) return true;
    if (agg->ncols > CRYO_AGG_MAX_COLS || agg->rsv != 0 || (agg->ncols > 0 && !cols)) return false;
    for (uint32_t j = 0; j < agg->ncols; j++)
        if (!agg_col_ok(f, atts, cols[j], max_att, true)) return false;
    *ncols = agg->ncols;
    return true;
}

static int group_pass(cryo_codec *c, int method, const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                      uint32_t B, uint64_t n, const GroupIo &io)
{
    static_assert(sizeof(cryo_group_block) == 2 * sizeof(uint4) && sizeof(cryo_group_rec) == 24 && sizeof(cryo_group) == 16,
                  "the grouping's records are the kernels'");
    const uint64_t S = cryo::filter_side_stride(B);
    DecodePass ps(d_src, d_src_off, d_src_size, true);
    ps.fixed = 256u;                                                 /* the six column slots */
    const uint32_t cpg = io.ncols + (uint32_t)__builtin_popcount(io.sd.text); /* a group's cells */
    ps.own_per_block = S * (sizeof(cryo_group_rec) + cpg * sizeof(cryo_agg_cell)); /* the side area */
    ps.run = [&](const DecodeChunk &ch) -> int {
        const void *slots = io.d_slots ? io.d_slots : ch.fixed;
        if (ch.lo == 0) {
            HIP_TRY(c, hipMemsetAsync(io.d_total, 0, sizeof(uint64_t), c->stream));
            if (!io.d_slots) {
                HIP_TRY(c, hipMemsetAsync(ch.fixed, 0, 48, c->stream));
                HIP_TRY(c, hipMemcpyAsync(ch.fixed, io.d_by, io.nby * sizeof(cryo_agg_col), hipMemcpyDeviceToDevice, c->stream));
                if (io.ncols)
                    HIP_TRY(c, hipMemcpyAsync(ch.fixed + 16, io.d_cols, io.ncols * sizeof(cryo_agg_col), hipMemcpyDeviceToDevice, c->stream));
            }
        }
        uint8_t *side_rec = ch.own, *side_cell = ch.own + ch.K * S * sizeof(cryo_group_rec);
        HIP_TRY(c, cryo::launch_group(scan_chunk(c, ch, B), io.sd,
                                      {.d_slots = slots, .nby = io.nby, .ncols = io.ncols, .d_blocks = (uint4 *)(io.d_blocks + ch.lo),
                                       .d_side_rec = side_rec, .d_side_cell = side_cell, .d_running = io.d_total, .d_rec = io.d_groups,
                                       .d_cells = io.d_cells, .group_cap = io.group_cap}));
        return CRYO_OK;
    };
    return decode_pass(c, method, B, n, ps);
}

/* ---- the projecting scan ----
 * The shared decode loop over the caller's stream table; on every decoded chunk project.hip tests the keys on every tuple and
 * writes a record per match and bad item and a row per match to a side area, places the blocks behind the two running totals --
 * which stay in device memory (d_total) from chunk to chunk -- and copies records and rows to their places in the call's output.
 * Per chunk (own) each block has 8 + row_bytes bytes per possible item of side area; the pass's fixed bytes hold the kernel's
 * column table when the caller's columns come as a device array.  The pass waits once, for that table, and then for nothing.
 * Its decodes count nowhere. */
namespace {
/* the kernel's column table (launch_project): {att, width, offset within the row, 0} per column, unused entries all zero */
struct ProjectTab {
    cryo_agg_col tab[CRYO_PROJECT_MAX_COLS] = {};
    uint32_t ncols = 0, row_bytes = 0;
};
struct ProjectIo {
    ScanDesc sd;
    ProjectTab pt;
    const void *d_tab = nullptr;            /* device: pt.tab in place already, or null: the pass uploads it */
    cryo_project_block *d_blocks = nullptr; /* device: n rows of the block table */
    void *d_rows = nullptr;                 /* device: row_cap rows */
    cryo_project_rec *d_rec = nullptr;      /* device: rec_cap records */
    uint64_t row_cap = 0, rec_cap = 0;
    uint64_t *d_total = nullptr;            /* device: the two running totals */
};
} // namespace

/* the projection's descriptor rules (include/cryo_codec.h); every array is host memory here.  *max_att: the highest key or
 * projected column; *pt: the kernel's column table and the row's size */
static bool project_desc_ok(const cryo_filter *f, const cryo_att *atts, const cryo_scan_key *keys, const cryo_project *prj,
                            const cryo_project_col *cols, uint32_t *max_att, ProjectTab *pt)
{
    if (!filter_desc_ok(f, atts, keys, max_att)) return false;
    if ((f->flags & ~CRYO_FILTER_TRUTH) != 0 || !prj || prj->ncols == 0 || prj->ncols > CRYO_PROJECT_MAX_COLS || prj->rsv != 0 || !cols) return false;
    *pt = ProjectTab();
    uint32_t end = 0;
    for (uint32_t j = 0; j < prj->ncols; j++) {
        const cryo_project_col &q = cols[j];
        if (q.rsv != 0 || q.rsv2 != 0 || q.att == 0 || q.att > f->natts) return false;
        const cryo_att &a = atts[q.att - 1];
        if ((a.attlen != 1 && a.attlen != 2 && a.attlen != 4 && a.attlen != 8) || a.attalign < a.attlen) return false;
        if (q.att > *max_att) *max_att = q.att;
        const uint32_t at = CRYO_PROJECT_COL_OFFSET(end, a.attlen);
        pt->tab[j].att = q.att;
        pt->tab[j].type = (uint8_t)a.attlen;
        pt->tab[j].rsv = (uint8_t)at;
        end = at + (uint32_t)a.attlen;
    }
    pt->ncols = prj->ncols;
    pt->row_bytes = CRYO_PROJECT_ROW_BYTES(end);
    return true;
}

static int project_pass(cryo_codec *c, int method, const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                        uint32_t B, uint64_t n, const ProjectIo &io)
{
    static_assert(sizeof(cryo_project_block) == 2 * sizeof(uint4) && sizeof(cryo_project_rec) == sizeof(uint2) &&
                      sizeof(cryo_project_col) == sizeof(cryo_agg_col) && sizeof(cryo_project) == 16,
                  "the projection's records are the kernels'");
    const uint64_t S = cryo::filter_side_stride(B);
    DecodePass ps(d_src, d_src_off, d_src_size, true);
    ps.fixed = 256u;                                                           /* the column table */
    ps.own_per_block = S * (sizeof(cryo_project_rec) + io.pt.row_bytes);       /* the side area */
    ps.run = [&](const DecodeChunk &ch) -> int {
        const void *tab = io.d_tab ? io.d_tab : ch.fixed;
        if (ch.lo == 0) {
            HIP_TRY(c, hipMemsetAsync(io.d_total, 0, 2 * sizeof(uint64_t), c->stream));
            if (!io.d_tab) { /* io is the call's own: the table is in place before the call goes on */
                HIP_TRY(c, hipMemcpyAsync(ch.fixed, io.pt.tab, sizeof io.pt.tab, hipMemcpyHostToDevice, c->stream));
                HIP_TRY(c, hipStreamSynchronize(c->stream));
            }
        }
        uint8_t *side_rec = ch.own, *side_rows = ch.own + ch.K * S * sizeof(cryo_project_rec);
        HIP_TRY(c, cryo::launch_project(scan_chunk(c, ch, B), io.sd,
                                        {.d_cols = tab, .ncols = io.pt.ncols, .row_bytes = io.pt.row_bytes, .d_blocks = (uint4 *)(io.d_blocks + ch.lo),
                                         .d_side_rec = side_rec, .d_side_rows = side_rows, .d_running = io.d_total, .d_rec = io.d_rec,
                                         .rec_cap = io.rec_cap, .d_rows = io.d_rows, .row_cap = io.row_cap}));
        return CRYO_OK;
    };
    return decode_pass(c, method, B, n, ps);
}

/* ---- the ordered scan ----
 * The shared decode loop over the caller's stream table; on every decoded chunk topn.hip tests the keys on every tuple, writes a
 * row per match to a side area, ranks each block's matches in LDS and writes a record and the row's side-area index per kept row,
 * places the blocks behind the running total -- which stays in device memory (*d_total) from chunk to chunk -- and gathers records
 * and rows to their places in the call's output.  Per chunk (own) each block has 24 + row_bytes + 4 bytes per possible item of
 * side area; the pass's fixed bytes hold the kernel's table -- the order columns, then the projection's column table -- when the
 * caller's arrays come as device arrays.  The pass waits once, for that table, and then for nothing.  Its decodes count nowhere. */
namespace {
/* the kernel's table (launch_topn): entries 0 .. 1 the order columns {att, type, flags, 0}, entries 2 .. 9 ProjectTab's */
struct TopnTab {
    cryo_agg_col slots[CRYO_ORDER_MAX_BY + CRYO_PROJECT_MAX_COLS] = {};
    uint32_t nby = 0, limit = 0, ncols = 0, row_bytes = 0;
};
struct TopnIo {
    ScanDesc sd;
    TopnTab tt;
    const void *d_tab = nullptr;         /* device: tt.slots in place already, or null: the pass uploads it */
    cryo_topn_block *d_blocks = nullptr; /* device: n rows of the block table */
    void *d_rows = nullptr;              /* device: row_cap rows */
    cryo_topn_rec *d_rec = nullptr;      /* device: row_cap records */
    uint64_t row_cap = 0;
    uint64_t *d_total = nullptr;         /* device: the running total */
};
} // namespace

/* the kept rows a block can have under `limit` */
static uint64_t topn_per_block(uint32_t limit, uint64_t side_stride) { return limit < side_stride ? limit : side_stride; }

/* the ordered scan's descriptor rules (include/cryo_codec.h); every array is host memory here.  *max_att: the highest key,
 * projected or order column; *tt: the kernel's table, the limit and the row's size */
static bool topn_desc_ok(const cryo_filter *f, const cryo_att *atts, const cryo_scan_key *keys, const cryo_order *ord,
                         const cryo_order_col *by, const cryo_project *prj, const cryo_project_col *cols, uint32_t *max_att, TopnTab *tt)
{
    ProjectTab pt;
    if (!project_desc_ok(f, atts, keys, prj, cols, max_att, &pt)) return false;
    if (!ord || ord->nby == 0 || ord->nby > CRYO_ORDER_MAX_BY || ord->limit == 0 || !by) return false;
    *tt = TopnTab();
    for (uint32_t j = 0; j < ord->nby; j++) {
        const cryo_order_col &q = by[j];
        if ((q.flags & ~(CRYO_ORDER_DESC | CRYO_ORDER_NULLS_FIRST)) != 0 || q.rsv != 0) return false;
        const cryo_agg_col as_col = {q.att, q.type, 0, 0};
        if (!agg_col_ok(f, atts, as_col, max_att, true)) return false;
        tt->slots[j] = {q.att, q.type, q.flags, 0};
    }
    memcpy(tt->slots + CRYO_ORDER_MAX_BY, pt.tab, sizeof pt.tab);
    tt->nby = ord->nby; tt->limit = ord->limit; tt->ncols = pt.ncols; tt->row_bytes = pt.row_bytes;
    return true;
}

static int topn_pass(cryo_codec *c, int method, const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                     uint32_t B, uint64_t n, const TopnIo &io)
{
    static_assert(sizeof(cryo_topn_block) == 2 * sizeof(uint4) && sizeof(cryo_topn_rec) == 24 && sizeof(cryo_order_col) == sizeof(cryo_agg_col) &&
                      sizeof(cryo_order) == 16,
                  "the ordered scan's records are the kernels'");
    const uint64_t S = cryo::filter_side_stride(B);
    DecodePass ps(d_src, d_src_off, d_src_size, true);
    ps.fixed = 256u;                                                                         /* the table */
    ps.own_per_block = (S * (sizeof(cryo_topn_rec) + io.tt.row_bytes + sizeof(uint32_t)) + 7u) & ~(uint64_t)7u; /* the side area */
    ps.run = [&](const DecodeChunk &ch) -> int {
        const void *tab = io.d_tab ? io.d_tab : ch.fixed;
        if (ch.lo == 0) {
            HIP_TRY(c, hipMemsetAsync(io.d_total, 0, sizeof(uint64_t), c->stream));
            if (!io.d_tab) { /* io is the call's own: the table is in place before the call goes on */
                HIP_TRY(c, hipMemcpyAsync(ch.fixed, io.tt.slots, sizeof io.tt.slots, hipMemcpyHostToDevice, c->stream));
                HIP_TRY(c, hipStreamSynchronize(c->stream));
            }
        }
        /* records and rows are whole words; the order list, of 4-byte entries, lies behind them */
        uint8_t *side_rec = ch.own, *side_rows = side_rec + ch.K * S * sizeof(cryo_topn_rec);
        uint8_t *side_ord = side_rows + ch.K * S * io.tt.row_bytes;
        HIP_TRY(c, cryo::launch_topn(scan_chunk(c, ch, B), io.sd,
                                     {.d_slots = tab, .h_slots = io.tt.slots, .nby = io.tt.nby, .ncols = io.tt.ncols, .row_bytes = io.tt.row_bytes,
                                      .limit = io.tt.limit, .d_blocks = (uint4 *)(io.d_blocks + ch.lo), .d_side_rec = side_rec,
                                      .d_side_rows = side_rows, .d_side_ord = side_ord, .d_running = io.d_total, .d_rec = io.d_rec,
                                      .d_rows = io.d_rows, .row_cap = io.row_cap}));
        return CRYO_OK;
    };
    return decode_pass(c, method, B, n, ps);
}

/* ---- recompression ----
 * The shared decode loop over the caller's stream table; every decoded chunk is encoded by cryo_codec_compress_batch -- the
 * path of every compress call, so the handle's encode options (segment mode, checksums, verification) apply as they are --
 * and recode.hip folds the two statuses of each block and, for the host-buffer call, packs the chunk's streams.  The pass
 * lives in c->d_rec, not in c->d_vfy: with verification on, the encode runs verify_pass, which decodes into c->d_vfy while this
 * pass still holds the decoded chunk.  Per chunk of K blocks the buffer holds the decoded blocks, the stream tables, and (own)
 * K output slots and a packed area of K slots for the host-buffer call, sizes, statuses and offsets; the encoder's workspace
 * (run_ws) shares c->d_ws with the decoders'.  With verification on, K also leaves room for the verifier's decoded copy of
 * the chunk, and while a chunk is encoded CRYO_OPT_WORKSPACE_MAX_BYTES is lowered by what this pass holds, so that the
 * verifier plans its own chunks within the rest. */
namespace {
struct RecodeOut {
    /* device-resident call: the caller's slots and arrays */
    uint8_t *d_dst = nullptr;
    uint64_t dst_stride = 0;
    uint32_t *d_out_size = nullptr;
    int32_t *d_status = nullptr;
    /* host-buffer call: stream i at h_dst + h_off[i] - h_base (h_off[i] counts from h_base on), within dst_cap bytes */
    uint8_t *h_dst = nullptr;
    size_t dst_cap = 0;
    uint64_t h_base = 0;
    uint64_t *h_off = nullptr;
    uint32_t *h_size = nullptr;
    int32_t *h_status = nullptr;
};
} // namespace

static int recode_pass(cryo_codec *c, int src_method, const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                       uint32_t B, uint64_t n, int dst_method, int dst_param, RecodeOut &out)
{
    const bool host = out.h_dst != nullptr;
    const uint64_t bound = cryo_codec_bound(dst_method, B);
    const uint64_t dstride = host ? (bound + 15u) & ~(uint64_t)15u : out.dst_stride;
    uint64_t h_run = 0; /* packed bytes of the chunks before this one */
    DecodePass ps(d_src, d_src_off, d_src_size, false);
    ps.buf = &c->d_rec; ps.cap = &c->rec_cap;
    ps.fixed = 256u;                                    /* the chunk's packed total (u64) */
    ps.own_per_block = (host ? 2u * dstride : 0u) + 32u; /* slots, packed area; size u32, status i32, K + 1 offsets u64 */
    ps.run_ws = [&](uint64_t K) { return encode_workspace(c, dst_method, dst_param, B, K); };
    if (c->verify) ps.elsewhere_per_block = (((uint64_t)B + 15u) & ~(uint64_t)15u) + 64u; /* verify_pass: decoded block, tables */
    ps.run = [&](const DecodeChunk &ch) -> int {
        uint8_t *slots = host ? ch.own : out.d_dst + ch.lo * dstride;
        uint8_t *packed = ch.own + ch.K * dstride;
        uint8_t *m = ch.own + (host ? 2u * ch.K * dstride : 0u);
        uint32_t *sz = host ? (uint32_t *)m : out.d_out_size + ch.lo;
        int32_t *st = host ? (int32_t *)(m + ch.K * 4u) : out.d_status + ch.lo;
        uint64_t *off = (uint64_t *)(m + ch.K * 8u);
        uint64_t *total = (uint64_t *)ch.fixed;
        /* the encode counts in cryo_codec_counters as any compress does; the decodes above counted no block */
        int rc;
        {
            struct WsMaxScope { /* the option is what it was on every way out */
                cryo_codec *c; size_t was;
                ~WsMaxScope() { c->ws_max = was; }
            } scope_{c, c->ws_max};
            if (c->ws_max) c->ws_max = c->ws_max > c->rec_cap ? c->ws_max - c->rec_cap : 1;
            rc = cryo_codec_compress_batch(c, dst_method, dst_param, ch.dec, ch.Bp, B, ch.cnt, slots, dstride, sz, st);
        }
        if (rc != CRYO_OK) return rc;
        HIP_TRY(c, cryo::launch_recode_offsets(c->stream, ch.cnt, dstride, ch.dec_st, st, sz, 0, off, total));
        if (!host) return CRYO_OK;
        HIP_TRY(c, cryo::launch_recode_pack(c->stream, ch.cnt, slots, dstride, sz, off, total, packed, c->lz4_opts.cus));
        /* the host sizes the copy of the packed bytes from the sizes: two waits per chunk */
        HIP_TRY(c, hipMemcpyAsync(out.h_size + ch.lo, sz, ch.cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(out.h_status + ch.lo, st, ch.cnt * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        uint64_t tot = 0;
        for (uint32_t k = 0; k < ch.cnt; k++) {
            const uint32_t s = out.h_size[ch.lo + k];
            if ((out.h_status[ch.lo + k] != CRYO_OK) != (s == 0) || s > bound) return CRYO_E_HIP;
            out.h_off[ch.lo + k] = out.h_base + h_run + tot;
            tot += ((uint64_t)s + 15u) & ~(uint64_t)15u;
        }
        c->xfer_ctr.d2h_bytes += tot + 8u * (uint64_t)ch.cnt;
        if (h_run + tot > out.dst_cap) return CRYO_E_DSTSIZE;
        if (tot) {
            HIP_TRY(c, hipMemcpyAsync(out.h_dst + h_run, packed, tot, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        h_run += tot;
        return CRYO_OK;
    };
    return decode_pass(c, src_method, B, n, ps);
}

static int recode_args(const cryo_codec *c, int src_method, int dst_method, int dst_param, size_t block_size)
{
    if (!c || !method_ok(src_method) || !method_ok(dst_method) || !block_size_ok(block_size)) return CRYO_E_ARG;
    if (dst_method == CRYO_METHOD_ZSTD && !cryo::zstd_compress_supported(dst_param, (uint32_t)block_size)) return CRYO_E_UNSUPPORTED;
    return CRYO_OK;
}

/* a host-buffer compress call found block `at` (index into the last verified batch) failed: its first differing byte, the
 * error text; `block` is the index the caller knows it by */
static void set_verify_failure(cryo_codec *c, uint64_t block, uint32_t off)
{
    c->vfy_failed = true;
    c->vfy_block = block;
    c->vfy_off = off;
    if (off == 0xffffffffu)
        snprintf(c->err, sizeof c->err, "block %llu failed verification: the decoders reject its stream", (unsigned long long)block);
    else
        snprintf(c->err, sizeof c->err, "block %llu failed verification at byte %u", (unsigned long long)block, off);
}
static int verify_failure(cryo_codec *c, uint64_t at)
{
    uint32_t off = 0xffffffffu;
    if (c->vfy_first) {
        HIP_TRY(c, hipMemcpyAsync(&off, c->vfy_first + at, sizeof off, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    set_verify_failure(c, at, off);
    return CRYO_E_VERIFY;
}
/* what the encoders said of n blocks, once statuses and sizes are on the host: the first block that did not come out right ends
 * the call; the sizes go to out_size (which may be `size` itself) */
static int take_encoded(cryo_codec *c, const int32_t *status, const uint32_t *size, size_t n, size_t bound, uint32_t *out_size)
{
    for (size_t i = 0; i < n; i++) {
        if (status[i] == CRYO_E_VERIFY) return verify_failure(c, i);
        if (status[i] != CRYO_OK) return status[i];
        if (size[i] == 0 || size[i] > bound) return CRYO_E_HIP;
        out_size[i] = size[i];
    }
    return CRYO_OK;
}

int cryo_codec_verify_batch(cryo_codec *c, int method, const void *d_raw, uint64_t raw_stride, uint32_t block_size,
                            uint64_t n_blocks, const void *d_comp, const uint64_t *d_comp_off, const uint32_t *d_comp_size,
                            int32_t *d_status, uint32_t *d_first_mismatch)
{
    DevGuard dev_(c);
    if (!c || !method_ok(method) || !block_size_ok(block_size)) return CRYO_E_ARG;
    if (n_blocks == 0) return CRYO_OK;
    if (!d_raw || !d_comp || !d_comp_off || !d_comp_size || !d_status || raw_stride < block_size) return CRYO_E_ARG;
    return guarded([&] {
        return verify_pass(c, method, (const uint8_t *)d_raw, raw_stride, block_size, n_blocks, (const uint8_t *)d_comp, d_comp_off,
                           0, d_comp_size, d_status, false, d_first_mismatch);
    });
}

int cryo_codec_check_batch(cryo_codec *c, int method, const void *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                           uint32_t block_size, uint64_t n_blocks, cryo_check_result *d_result)
{
    DevGuard dev_(c);
    if (!c || !method_ok(method) || !check_block_size_ok(block_size)) return CRYO_E_ARG;
    if (n_blocks == 0) return CRYO_OK;
    if (!d_src || !d_src_off || !d_src_size || !d_result) return CRYO_E_ARG;
    return guarded([&] {
        return check_pass(c, method, (const uint8_t *)d_src, d_src_off, d_src_size, block_size, n_blocks, d_result);
    });
}

int cryo_codec_fetch_batch(cryo_codec *c, int method, const void *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                           uint32_t block_size, uint64_t n_blocks, const uint64_t *d_req_first, const uint16_t *d_pos, uint64_t n_req,
                           void *d_dst, uint64_t dst_cap, cryo_fetch_result *d_result, uint64_t *d_total)
{
    DevGuard dev_(c);
    if (!c || !method_ok(method) || !check_block_size_ok(block_size)) return CRYO_E_ARG;
    if (!d_total || ((uintptr_t)d_total & 7u) != 0) return CRYO_E_ARG;
    if (n_blocks == 0) {
        HIP_TRY(c, hipMemsetAsync(d_total, 0, sizeof(uint64_t), c->stream));
        return CRYO_OK;
    }
    if (!d_src || !d_src_off || !d_src_size || !d_req_first || ((uintptr_t)d_req_first & 7u) != 0) return CRYO_E_ARG;
    if (n_req > 0 && (!d_pos || !d_result)) return CRYO_E_ARG;
    if ((!d_dst && dst_cap > 0) || ((uintptr_t)d_dst & 7u) != 0 || ((uintptr_t)d_result & 15u) != 0) return CRYO_E_ARG;
    return guarded([&] {
        FetchIo io;
        io.d_req_first = d_req_first; io.d_pos = d_pos; io.n_req = n_req; io.d_result = d_result;
        io.d_dst = (uint8_t *)d_dst; io.dst_cap = dst_cap; io.d_total = d_total;
        return fetch_pass(c, method, (const uint8_t *)d_src, d_src_off, d_src_size, block_size, n_blocks, io);
    });
}

/* The descriptor of a device-resident scan call: f and, where the call has them, grp and agg (need_agg: the call is nothing
 * without aggregate columns) are host structs whose arrays live in device memory.  In this order: the pointer and alignment
 * rules of the structs, which touch no device; the arrays read back and held against the call's *_desc_ok before anything else
 * is queued; the call's totals (total_words of them at d_total; none: 0) cleared; and -- unless the call has no block -- the key
 * table of a descriptor with a byte-string key (key_table_device: without such a key nothing more is queued) and the bucket table
 * of a CRYO_GROUP_BUCKETS group descriptor, whose buckets array is read back beside by (bucket_table_device).  *ncols: the
 * aggregate columns.  prj: the call is a projection (grp and agg null); *pt: its column table.  ord (with prj): the call is an
 * ordered scan; *tt: its table, and pt is not looked at */
static int scan_desc_device(cryo_codec *c, const cryo_filter *f, const cryo_group *grp, const cryo_agg *agg, bool need_agg,
                            uint64_t *d_total, size_t total_words, uint64_t n_blocks, ScanDesc &sd, uint32_t *ncols,
                            const cryo_project *prj = nullptr, ProjectTab *pt = nullptr, const cryo_order *ord = nullptr,
                            TopnTab *tt = nullptr)
{
    if (!f || f->natts == 0 || f->natts > CRYO_FILTER_MAX_ATTS || f->nkeys > CRYO_FILTER_MAX_KEYS || !f->atts ||
        (f->nkeys > 0 && !f->keys) || ((uintptr_t)f->atts & 3u) != 0 || ((uintptr_t)f->keys & 7u) != 0)
        return CRYO_E_ARG;
    if (grp && (grp->nby == 0 || grp->nby > CRYO_GROUP_MAX_BY || !grp->by || ((uintptr_t)grp->by & 7u) != 0)) return CRYO_E_ARG;
    if (grp && (!group_rsv_ok(grp->rsv) ||
                (grp->rsv == CRYO_GROUP_BUCKETS && (!group_buckets(grp) || ((uintptr_t)group_buckets(grp) & 7u) != 0))))
        return CRYO_E_ARG;
    const cryo_bucket *d_bk = grp ? group_buckets(grp) : nullptr; /* device */
    const uint32_t nc = agg ? agg->ncols : 0u;
    if ((need_agg && nc == 0) || nc > CRYO_AGG_MAX_COLS || (nc > 0 && (!agg->cols || ((uintptr_t)agg->cols & 7u) != 0)))
        return CRYO_E_ARG;
    if (prj && (prj->ncols == 0 || prj->ncols > CRYO_PROJECT_MAX_COLS || !prj->cols || ((uintptr_t)prj->cols & 7u) != 0)) return CRYO_E_ARG;
    if (ord && (ord->nby == 0 || ord->nby > CRYO_ORDER_MAX_BY || ord->limit == 0 || !ord->by || ((uintptr_t)ord->by & 7u) != 0)) return CRYO_E_ARG;
    cryo_order_col ocols[CRYO_ORDER_MAX_BY];
    cryo_att atts[CRYO_FILTER_MAX_ATTS]; /* 6 400 bytes */
    cryo_scan_key keys[CRYO_FILTER_MAX_KEYS];
    cryo_agg_col by[CRYO_GROUP_MAX_BY], cols[CRYO_AGG_MAX_COLS];
    cryo_bucket bk[CRYO_GROUP_MAX_BY];
    cryo_project_col pcols[CRYO_PROJECT_MAX_COLS];
    HIP_TRY(c, hipMemcpyAsync(atts, f->atts, f->natts * sizeof(cryo_att), hipMemcpyDeviceToHost, c->stream));
    if (f->nkeys)
        HIP_TRY(c, hipMemcpyAsync(keys, f->keys, f->nkeys * sizeof(cryo_scan_key), hipMemcpyDeviceToHost, c->stream));
    if (grp) HIP_TRY(c, hipMemcpyAsync(by, grp->by, grp->nby * sizeof(cryo_agg_col), hipMemcpyDeviceToHost, c->stream));
    if (d_bk) HIP_TRY(c, hipMemcpyAsync(bk, d_bk, grp->nby * sizeof(cryo_bucket), hipMemcpyDeviceToHost, c->stream));
    if (nc) HIP_TRY(c, hipMemcpyAsync(cols, agg->cols, nc * sizeof(cryo_agg_col), hipMemcpyDeviceToHost, c->stream));
    if (prj) HIP_TRY(c, hipMemcpyAsync(pcols, prj->cols, prj->ncols * sizeof(cryo_project_col), hipMemcpyDeviceToHost, c->stream));
    if (ord) HIP_TRY(c, hipMemcpyAsync(ocols, ord->by, ord->nby * sizeof(cryo_order_col), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *ncols = nc;
    const bool ok = ord        ? topn_desc_ok(f, atts, keys, ord, ocols, prj, pcols, &sd.max_att, tt)
                    : prj      ? project_desc_ok(f, atts, keys, prj, pcols, &sd.max_att, pt)
                    : grp      ? group_desc_ok(f, atts, keys, grp, by, d_bk ? bk : nullptr, agg, cols, &sd.max_att, ncols, &sd.text)
                    : need_agg ? agg_desc_ok(f, atts, keys, agg, cols, &sd.max_att)
                               : filter_desc_ok(f, atts, keys, &sd.max_att);
    if (!ok) return CRYO_E_ARG;
    if (total_words) HIP_TRY(c, hipMemsetAsync(d_total, 0, total_words * sizeof(uint64_t), c->stream));
    if (n_blocks == 0) return CRYO_OK;
    sd.d_atts = f->atts; sd.d_keys = f->keys; sd.nkeys = f->nkeys;
    bool table_keys = false;
    int rc = key_table_device(c, keys, f->nkeys, &sd.d_keys, &table_keys);
    if (rc == CRYO_OK && d_bk) rc = bucket_table_device(c, bk, grp->nby, &sd.d_buckets);
    sd.floats = desc_has_float(keys, f->nkeys, cols, *ncols);
    sd.like = desc_has_like(keys, f->nkeys);
    sd.truth = scan_truth(f, table_keys || sd.floats || d_bk || sd.text); /* the bucket and the text kernels have the table's verdict path alone */
    return rc;
}

int cryo_codec_filter_batch(cryo_codec *c, int method, const void *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                            uint32_t block_size, uint64_t n_blocks, const cryo_filter *f, void *d_dst, uint64_t dst_cap,
                            cryo_filter_rec *d_rec, uint64_t rec_cap, cryo_filter_block *d_blocks, uint64_t *d_total)
{
    DevGuard dev_(c);
    if (!c || !method_ok(method) || !check_block_size_ok(block_size)) return CRYO_E_ARG;
    if (!d_total || ((uintptr_t)d_total & 7u) != 0) return CRYO_E_ARG;
    const bool count_only = f && (f->flags & CRYO_FILTER_COUNT_ONLY) != 0;
    if (n_blocks > 0) {
        if (!d_src || !d_src_off || !d_src_size || !d_blocks || ((uintptr_t)d_blocks & 15u) != 0) return CRYO_E_ARG;
        if (!count_only && ((!d_dst && dst_cap > 0) || (!d_rec && rec_cap > 0))) return CRYO_E_ARG;
        if ((((uintptr_t)d_dst | (uintptr_t)d_rec) & 7u) != 0) return CRYO_E_ARG;
    }
    return guarded([&] {
        FilterIo io;
        uint32_t ncols = 0;
        const int rc = scan_desc_device(c, f, nullptr, nullptr, false, d_total, 2, n_blocks, io.sd, &ncols);
        if (rc != CRYO_OK || n_blocks == 0) return rc;
        io.count_only = count_only;
        io.d_blocks = d_blocks; io.dst_cap = count_only ? 0 : dst_cap; io.rec_cap = count_only ? 0 : rec_cap;
        io.d_dst = (uint8_t *)d_dst; io.d_rec = d_rec; io.d_total = d_total;
        return filter_pass(c, method, (const uint8_t *)d_src, d_src_off, d_src_size, block_size, n_blocks, io);
    });
}

int cryo_codec_agg_batch(cryo_codec *c, int method, const void *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                         uint32_t block_size, uint64_t n_blocks, const cryo_filter *f, const cryo_agg *agg,
                         cryo_agg_block *d_blocks, cryo_agg_cell *d_cells)
{
    DevGuard dev_(c);
    if (!c || !method_ok(method) || !check_block_size_ok(block_size)) return CRYO_E_ARG;
    if (n_blocks > 0 && (!d_src || !d_src_off || !d_src_size || !d_blocks || !d_cells || ((uintptr_t)d_blocks & 15u) != 0 ||
                         ((uintptr_t)d_cells & 7u) != 0))
        return CRYO_E_ARG;
    return guarded([&] {
        AggIo io;
        const int rc = scan_desc_device(c, f, nullptr, agg, true, nullptr, 0, n_blocks, io.sd, &io.ncols);
        if (rc != CRYO_OK || n_blocks == 0) return rc;
        io.d_cols = agg->cols;
        io.d_blocks = d_blocks; io.d_cells = d_cells;
        return agg_pass(c, method, (const uint8_t *)d_src, d_src_off, d_src_size, block_size, n_blocks, io);
    });
}

int cryo_codec_group_batch(cryo_codec *c, int method, const void *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                           uint32_t block_size, uint64_t n_blocks, const cryo_filter *f, const cryo_group *grp, const cryo_agg *agg,
                           cryo_group_block *d_blocks, cryo_group_rec *d_groups, uint64_t group_cap, cryo_agg_cell *d_cells,
                           uint64_t *d_total)
{
    DevGuard dev_(c);
    if (!c || !method_ok(method) || !check_block_size_ok(block_size)) return CRYO_E_ARG;
    if (!d_total || ((uintptr_t)d_total & 7u) != 0 || !grp) return CRYO_E_ARG;
    const uint32_t ncols = agg ? agg->ncols : 0u;
    if ((((uintptr_t)d_groups | (uintptr_t)d_cells) & 7u) != 0 || ((uintptr_t)d_blocks & 15u) != 0) return CRYO_E_ARG;
    if (n_blocks > 0 && (!d_src || !d_src_off || !d_src_size || !d_blocks || (group_cap > 0 && (!d_groups || (ncols > 0 && !d_cells)))))
        return CRYO_E_ARG;
    return guarded([&] {
        GroupIo io;
        const int rc = scan_desc_device(c, f, grp, agg, false, d_total, 1, n_blocks, io.sd, &io.ncols);
        if (rc != CRYO_OK || n_blocks == 0) return rc;
        if (io.sd.text && group_cap > 0 && !d_cells) return (int)CRYO_E_ARG; /* the key cells need the room that ncols == 0 does not */
        io.d_by = grp->by; io.d_cols = ncols ? agg->cols : nullptr; io.nby = grp->nby;
        io.d_blocks = d_blocks; io.d_groups = d_groups; io.d_cells = d_cells; io.group_cap = group_cap; io.d_total = d_total;
        return group_pass(c, method, (const uint8_t *)d_src, d_src_off, d_src_size, block_size, n_blocks, io);
    });
}

int cryo_codec_project_batch(cryo_codec *c, int method, const void *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                             uint32_t block_size, uint64_t n_blocks, const cryo_filter *f, const cryo_project *prj, void *d_rows,
                             uint64_t row_cap, cryo_project_rec *d_rec, uint64_t rec_cap, cryo_project_block *d_blocks,
                             uint64_t *d_total)
{
    DevGuard dev_(c);
    if (!c || !method_ok(method) || !check_block_size_ok(block_size)) return CRYO_E_ARG;
    if (!d_total || ((uintptr_t)d_total & 7u) != 0 || !prj) return CRYO_E_ARG;
    if ((((uintptr_t)d_rows | (uintptr_t)d_rec) & 7u) != 0 || ((uintptr_t)d_blocks & 15u) != 0) return CRYO_E_ARG;
    if (n_blocks > 0 && (!d_src || !d_src_off || !d_src_size || !d_blocks || (!d_rows && row_cap > 0) || (!d_rec && rec_cap > 0)))
        return CRYO_E_ARG;
    return guarded([&] {
        ProjectIo io;
        uint32_t ncols = 0;
        const int rc = scan_desc_device(c, f, nullptr, nullptr, false, d_total, 2, n_blocks, io.sd, &ncols, prj, &io.pt);
        if (rc != CRYO_OK || n_blocks == 0) return rc;
        io.d_blocks = d_blocks; io.d_rows = d_rows; io.row_cap = row_cap; io.d_rec = d_rec; io.rec_cap = rec_cap; io.d_total = d_total;
        return project_pass(c, method, (const uint8_t *)d_src, d_src_off, d_src_size, block_size, n_blocks, io);
    });
}

int cryo_codec_topn_batch(cryo_codec *c, int method, const void *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                          uint32_t block_size, uint64_t n_blocks, const cryo_filter *f, const cryo_order *ord, const cryo_project *prj,
                          void *d_rows, cryo_topn_rec *d_rec, uint64_t row_cap, cryo_topn_block *d_blocks, uint64_t *d_total)
{
    DevGuard dev_(c);
    if (!c || !method_ok(method) || !check_block_size_ok(block_size)) return CRYO_E_ARG;
    if (!d_total || ((uintptr_t)d_total & 7u) != 0 || !prj || !ord) return CRYO_E_ARG;
    if ((((uintptr_t)d_rows | (uintptr_t)d_rec) & 7u) != 0 || ((uintptr_t)d_blocks & 15u) != 0) return CRYO_E_ARG;
    if (n_blocks > 0 && (!d_src || !d_src_off || !d_src_size || !d_blocks || ((!d_rows || !d_rec) && row_cap > 0))) return CRYO_E_ARG;
    return guarded([&] {
        TopnIo io;
        uint32_t ncols = 0;
        const int rc = scan_desc_device(c, f, nullptr, nullptr, false, d_total, 1, n_blocks, io.sd, &ncols, prj, nullptr, ord, &io.tt);
        if (rc != CRYO_OK || n_blocks == 0) return rc;
        io.d_blocks = d_blocks; io.d_rows = d_rows; io.d_rec = d_rec; io.row_cap = row_cap; io.d_total = d_total;
        return topn_pass(c, method, (const uint8_t *)d_src, d_src_off, d_src_size, block_size, n_blocks, io);
    });
}

int cryo_codec_recode_batch(cryo_codec *c, int src_method, const void *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                            uint32_t block_size, uint64_t n_blocks, int dst_method, int dst_param, void *d_dst, uint64_t dst_stride,
                            uint32_t *d_out_size, int32_t *d_status)
{
    DevGuard dev_(c);
    const int ok = recode_args(c, src_method, dst_method, dst_param, block_size);
    if (ok != CRYO_OK) return ok;
    if (n_blocks == 0) return CRYO_OK;
    if (!d_src || !d_src_off || !d_src_size || !d_dst || !d_out_size || !d_status) return CRYO_E_ARG;
    if (dst_stride < cryo_codec_bound(dst_method, block_size)) return CRYO_E_DSTSIZE;
    return guarded([&] {
        RecodeOut out;
        out.d_dst = (uint8_t *)d_dst; out.dst_stride = dst_stride; out.d_out_size = d_out_size; out.d_status = d_status;
        return recode_pass(c, src_method, (const uint8_t *)d_src, d_src_off, d_src_size, block_size, n_blocks, dst_method,
                           dst_param, out);
    });
}

int cryo_codec_last_verify_failure(const cryo_codec *c, uint64_t *block, uint32_t *first_mismatch)
{
    if (!c) return CRYO_E_ARG;
    if (!c->vfy_failed) return 0;
    if (block) *block = c->vfy_block;
    if (first_mismatch) *first_mismatch = c->vfy_off;
    return 1;
}

/* ---- single block, host buffers ---- */
int cryo_codec_compress_block(cryo_codec *c, int method, int param, const void *h_src,
                              size_t block_size, void *h_dst, size_t dst_cap, size_t *out_size)
{
    DevGuard dev_(c);
    if (!c || !h_src || !h_dst || !out_size || !method_ok(method)) return CRYO_E_ARG;
    if (!block_size_ok(block_size)) return CRYO_E_ARG;
    const size_t bound = cryo_codec_bound(method, block_size);
    if (dst_cap < bound) return CRYO_E_DSTSIZE;
    int rc;
    if ((rc = ensure(c, &c->d_in, &c->in_cap, block_size)) != CRYO_OK) return rc;
    if ((rc = ensure(c, &c->d_out, &c->out_cap, bound)) != CRYO_OK) return rc;
    c->vfy_failed = false;
    HIP_TRY(c, hipMemcpyAsync(c->d_in, h_src, block_size, hipMemcpyHostToDevice, c->stream));
    rc = cryo_codec_compress_batch(c, method, param, c->d_in, block_size, (uint32_t)block_size, 1,
                                   c->d_out, bound, c->d_size, c->d_status);
    if (rc != CRYO_OK) return rc;
    uint32_t csize = 0;
    int32_t st = 0;
    HIP_TRY(c, hipMemcpyAsync(&csize, c->d_size, sizeof csize, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&st, c->d_status, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((rc = take_encoded(c, &st, &csize, 1, bound, &csize)) != CRYO_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(h_dst, c->d_out, csize, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *out_size = csize;
    return CRYO_OK;
}

int cryo_codec_decompress_block(cryo_codec *c, int method, const void *h_src, size_t src_size,
                                void *h_dst, size_t block_size)
{
    DevGuard dev_(c);
    if (!c || !h_src || !h_dst || !method_ok(method)) return CRYO_E_ARG;
    if (!block_size_ok(block_size)) return CRYO_E_ARG;
    if (src_size == 0 || src_size > 0xFFFFFFFFu) return CRYO_E_CORRUPT;
    int rc;
    if ((rc = ensure(c, &c->d_in, &c->in_cap, src_size)) != CRYO_OK) return rc;
    if ((rc = ensure(c, &c->d_out, &c->out_cap, block_size)) != CRYO_OK) return rc;
    const uint64_t off = 0;
    const uint32_t sz = (uint32_t)src_size;
    HIP_TRY(c, hipMemcpyAsync(c->d_in, h_src, src_size, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_off, &off, sizeof off, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_size, &sz, sizeof sz, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); /* off/sz are stack variables */
    rc = cryo_codec_decompress_batch(c, method, c->d_in, c->d_off, c->d_size, c->d_out, block_size,
                                     (uint32_t)block_size, 1, c->d_status);
    if (rc != CRYO_OK) return rc;
    int32_t st = 0;
    HIP_TRY(c, hipMemcpyAsync(&st, c->d_status, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (st != CRYO_OK) return st;
    HIP_TRY(c, hipMemcpyAsync(h_dst, c->d_out, block_size, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CRYO_OK;
}

/* ---- K blocks, host buffers ---- */
} /* extern "C" */

/* ---- pipelined K-block calls -------------------------------------------------------------------------------
 * A call with tens of megabytes is cut into chunks; while chunk c runs on the GPU, chunk c+1 is gathered into a
 * pinned buffer by a few host threads and chunk c-1 travels back on a second stream and is scattered to the
 * caller's memory.  One chunk's life: host gather -> H2D (codec stream) -> kernel(s) (codec stream) -> D2H
 * (transfer stream) -> host scatter.  The one-shot path (one H2D of everything, the kernel, one D2H from pageable
 * memory, single-threaded copies) reached 13-19 GB/s on 4096 x 128 KiB, a quarter of the link. */
/* the chunk cut and the staged-stream layout are stated in host_stage.h */
static bool pipe_worth_it(const cryo_codec *c, size_t n, size_t block_size) { return n * block_size >= c->pipe_min_bytes && n >= 128; }
/* the four pinned staging buffers of the pipelined calls are K x block_size each: a 4096 x 1 MiB call leaves 2.3 GB of
 * pinned host memory behind.  What exceeds this cap is given back when the call ends. */
static void pipe_trim(cryo_codec *c)
{
    constexpr size_t kKeep = (size_t)256 << 20;
    for (int i = 0; i < 4; i++)
        if (c->pipe_pin_cap[i] > kKeep) { (void)hipHostFree(c->pipe_pin[i]); c->pipe_pin[i] = nullptr; c->pipe_pin_cap[i] = 0; }
}
/* a pipelined body: an error return must not leave copies in flight into the handle's pinned buffers or the caller's memory */
template <class Body> static int piped(cryo_codec *c, Body body)
{
    const int rc = body();
    if (rc != CRYO_OK) { (void)hipStreamSynchronize(c->stream); if (c->xfer) (void)hipStreamSynchronize(c->xfer); }
    pipe_trim(c);
    return rc;
}
/* the return leg of a pipelined call whose kernel has run over the whole call: the D2H of chunk c+1 (bytes(c+1) from its first
 * slot, the slots d_stride apart) on the transfer stream under landed(c), which waits for chunk c's event and scatters it */
template <class Bytes, class Landed> static int pipe_return(cryo_codec *c, const cryo::ChunkCut &cut, const uint8_t *d_from, size_t d_stride, Bytes bytes, Landed landed)
{
    auto d2h = [&](size_t ch) -> int {
        HIP_TRY(c, hipMemcpyAsync(c->pipe_pin[2 + (ch & 1)], d_from + cut.lo(ch) * d_stride, bytes(ch), hipMemcpyDeviceToHost, c->xfer));
        HIP_TRY(c, hipEventRecord(c->ev_out[ch & 1], c->xfer));
        return CRYO_OK;
    };
    int rc;
    if ((rc = d2h(0)) != CRYO_OK) return rc;
    for (size_t ch = 0; ch < cut.chunks(); ch++) {
        if (ch + 1 < cut.chunks() && (rc = d2h(ch + 1)) != CRYO_OK) return rc; /* its buffer was scattered in the previous turn */
        if ((rc = landed(ch)) != CRYO_OK) return rc;
    }
    return CRYO_OK;
}
/* decoded blocks, block_size apart from `from` (pinned memory, or the device: then the copies are queued on the codec stream), to
 * one destination each: a block that failed leaves its destination untouched, an OK block without one is the caller's error */
static int hand_back(cryo_codec *c, const int32_t *status, void *const *dst, const uint8_t *from, bool from_device, size_t n, size_t block_size)
{
    std::vector<CopyJob> jobs;
    for (size_t i = 0; i < n; i++) {
        if (status[i] != CRYO_OK) continue;
        if (!dst[i]) return CRYO_E_ARG;
        if (from_device) HIP_TRY(c, hipMemcpyAsync(dst[i], from + i * block_size, block_size, hipMemcpyDeviceToHost, c->stream));
        else jobs.push_back({dst[i], from + i * block_size, block_size});
    }
    parallel_copy(c, jobs);
    return CRYO_OK;
}

/* ---- compress: K blocks from / to host memory ---- */
/* the host blocks of a compress call: contiguous (block i at src + i * block_size, its slot at dst + i * dst_stride), or -- a
 * multi-GPU share, where a handle's blocks are every G-th of the call -- one pointer per block */
struct CompressIo {
    const uint8_t *src; uint8_t *dst; size_t dst_stride;
    const void *const *src_each; void *const *dst_each;
    bool contiguous() const { return !src_each; }
    void *out(size_t i) const { return dst_each ? dst_each[i] : dst + i * dst_stride; }
};

static int compress_blocks_piped(cryo_codec *c, int method, int param, const CompressIo &io, size_t block_size, size_t n, uint32_t *h_out_size)
{
    const size_t bound = cryo_codec_bound(method, block_size);
    const size_t dstride = (bound + 15) & ~(size_t)15;
    const cryo::ChunkCut cut(n, block_size);
    int rc;
    if ((rc = ensure_pipe_streams(c)) != CRYO_OK) return rc;
    if ((rc = ensure(c, &c->hb_src, &c->hb_src_cap, n * block_size + 64)) != CRYO_OK) return rc;
    if ((rc = ensure(c, &c->hb_dst, &c->hb_dst_cap, n * dstride + 64)) != CRYO_OK) return rc;
    if ((rc = ensure(c, &c->hb_meta, &c->hb_meta_cap, n * 16 + 64)) != CRYO_OK) return rc;
    if ((rc = ensure_pinned(c, n * 8 + 64)) != CRYO_OK) return rc;
    for (int b = 0; b < 2; b++) {
        if ((rc = ensure_pipe(c, b, cut.K * block_size)) != CRYO_OK) return rc;
        if ((rc = ensure_pipe(c, 2 + b, cut.K * dstride)) != CRYO_OK) return rc;
    }
    uint32_t *d_sz = (uint32_t *)c->hb_meta;
    int32_t *d_st = (int32_t *)(c->hb_meta + ((n * 4 + 15) & ~(size_t)15));
    uint32_t *p_sz = (uint32_t *)c->pin;
    int32_t *p_st = (int32_t *)((uint8_t *)c->pin + n * 4);
    for (size_t ch = 0; ch < cut.chunks(); ch++) {
        const size_t lo = cut.lo(ch), cnt = cut.cnt(ch);
        uint8_t *buf = (uint8_t *)c->pipe_pin[ch & 1];
        if (ch >= 2) HIP_TRY(c, hipEventSynchronize(c->ev_in[ch & 1])); /* the staging buffer has left for the device */
        std::vector<CopyJob> jobs;
        if (io.contiguous()) jobs.push_back({buf, io.src + lo * block_size, cnt * block_size});
        else for (size_t i = 0; i < cnt; i++) jobs.push_back({buf + i * block_size, io.src_each[lo + i], block_size});
        parallel_copy(c, jobs); /* the host gather of chunk c+1 overlaps the H2D of chunk c */
        HIP_TRY(c, hipMemcpyAsync(c->hb_src + lo * block_size, buf, cnt * block_size, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipEventRecord(c->ev_in[ch & 1], c->stream));
    }
    rc = cryo_codec_compress_batch(c, method, param, c->hb_src, block_size, (uint32_t)block_size, n, c->hb_dst, dstride, d_sz, d_st);
    if (rc != CRYO_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(c, hipMemcpyAsync(p_sz, d_sz, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(p_st, d_st, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((rc = take_encoded(c, p_st, p_sz, n, bound, h_out_size)) != CRYO_OK) return rc;
    /* out: only the bytes the blocks occupy travel */
    return pipe_return(c, cut, c->hb_dst, dstride, [&](size_t ch) { return (cut.cnt(ch) - 1) * dstride + p_sz[cut.hi(ch) - 1]; },
        [&](size_t ch) -> int {
            HIP_TRY(c, hipEventSynchronize(c->ev_out[ch & 1]));
            const uint8_t *po = (const uint8_t *)c->pipe_pin[2 + (ch & 1)];
            std::vector<CopyJob> jobs;
            for (size_t i = cut.lo(ch); i < cut.hi(ch); i++) jobs.push_back({io.out(i), po + (i - cut.lo(ch)) * dstride, p_sz[i]});
            parallel_copy(c, jobs);
            return (int)CRYO_OK;
        });
}

/* Device buffers and the pinned staging buffer live in the handle (grow-only).  A large call takes the pipeline; else contiguous
 * blocks go up straight from the caller's memory, and blocks given by pointer go through the pinned buffer both ways, on the
 * worker threads.  The caller has checked the arguments */
static int compress_blocks_host(cryo_codec *c, int method, int param, const CompressIo &io, size_t block_size, size_t n, uint32_t *h_out_size)
{
    DevGuard dev_(c);
    if (n == 0) return CRYO_OK;
    const size_t bound = cryo_codec_bound(method, block_size);
    ScopedLocalCpus numa_(c, n, block_size); /* the caller's share of the copies next to the GPU */
    c->vfy_failed = false;
    if (pipe_worth_it(c, n, block_size))
        return piped(c, [&] { return compress_blocks_piped(c, method, param, io, block_size, n, h_out_size); });
    /* bulk: the device slots use the caller's stride, so the output goes back in one copy (a slot may be written beyond
     * out_size[i], up to bound) */
    const bool bulk = io.contiguous() && io.dst_stride <= bound + 4096;
    const size_t dstride = bulk ? io.dst_stride : ((bound + 15) & ~(size_t)15);
    int rc;
    if ((rc = ensure(c, &c->hb_src, &c->hb_src_cap, n * block_size + 64)) != CRYO_OK) return rc;
    if ((rc = ensure(c, &c->hb_dst, &c->hb_dst_cap, n * dstride + 64)) != CRYO_OK) return rc;
    if ((rc = ensure(c, &c->hb_meta, &c->hb_meta_cap, n * 16 + 64)) != CRYO_OK) return rc;
    uint32_t *d_sz = (uint32_t *)c->hb_meta;
    int32_t *d_st = (int32_t *)(c->hb_meta + ((n * 4 + 15) & ~(size_t)15));
    /* pinned: the statuses; by pointer the blocks of both directions before them (dstride >= block_size) and the sizes behind */
    if ((rc = ensure_pinned(c, io.contiguous() ? n * 4 : n * dstride + n * 8 + 64)) != CRYO_OK) return rc;
    uint8_t *pin = (uint8_t *)c->pin;
    int32_t *h_st = (int32_t *)(io.contiguous() ? pin : pin + n * dstride);
    uint32_t *h_sz = io.contiguous() ? h_out_size : (uint32_t *)(pin + n * dstride + n * 4);
    if (!io.contiguous()) {
        std::vector<CopyJob> jobs;
        for (size_t i = 0; i < n; i++) jobs.push_back({pin + i * block_size, io.src_each[i], block_size});
        parallel_copy(c, jobs);
    }
    HIP_TRY(c, hipMemcpyAsync(c->hb_src, io.contiguous() ? io.src : pin, n * block_size, hipMemcpyHostToDevice, c->stream));
    rc = cryo_codec_compress_batch(c, method, param, c->hb_src, block_size, (uint32_t)block_size, n, c->hb_dst, dstride, d_sz, d_st);
    if (rc != CRYO_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(c, hipMemcpyAsync(h_sz, d_sz, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_st, d_st, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    /* a padded stride: rows of `bound` bytes, so that the caller's bytes between the slots stay the caller's */
    if (bulk && dstride == bound) HIP_TRY(c, hipMemcpyAsync(io.dst, c->hb_dst, n * bound, hipMemcpyDeviceToHost, c->stream));
    else if (bulk) HIP_TRY(c, hipMemcpy2DAsync(io.dst, dstride, c->hb_dst, dstride, bound, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((rc = take_encoded(c, h_st, h_sz, n, bound, h_out_size)) != CRYO_OK) return rc;
    if (bulk) return CRYO_OK;
    if (io.contiguous()) {
        for (size_t i = 0; i < n; i++)
            HIP_TRY(c, hipMemcpyAsync(io.out(i), c->hb_dst + i * dstride, h_out_size[i], hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return CRYO_OK;
    }
    /* the compressed blocks come back in ONE copy into the pinned buffer (its input side is no longer needed) and go to
     * their destinations from there on the worker threads; round 3 copied block by block into pageable memory */
    HIP_TRY(c, hipMemcpyAsync(pin, c->hb_dst, (n - 1) * dstride + h_out_size[n - 1], hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<CopyJob> jobs;
    for (size_t i = 0; i < n; i++) jobs.push_back({io.out(i), pin + i * dstride, h_out_size[i]});
    parallel_copy(c, jobs);
    return CRYO_OK;
}

/* ---- decompress and check: streams given by pointer, staged for the device ---- */
/* a stream with bytes needs a place to read them from */
static bool streams_ok(const void *const *h_src, const uint32_t *h_src_size, size_t n)
{
    for (size_t i = 0; i < n; i++) if (h_src_size[i] != 0 && !h_src[i]) return false;
    return true;
}
/* the whole of layout L (host_stage.h) written at `at`: the two tables, and stream k's bytes from src_of(k).  spread: the copies go
 * over the staging workers */
template <class SrcOf, class SizeOf> static void write_staged(cryo_codec *c, const cryo::StreamLayout &L, uint8_t *at, SrcOf src_of, SizeOf size_of, bool spread)
{
    L.fill_tables(at, size_of);
    std::vector<CopyJob> jobs;
    for (size_t k = 0; k < L.m; k++) {
        if (!size_of(k)) continue;
        if (spread) jobs.push_back({at + L.offset(k), src_of(k), size_of(k)});
        else memcpy(at + L.offset(k), src_of(k), size_of(k));
    }
    parallel_copy(c, jobs);
}
/* the one-shot staging of n streams given by pointer: the layout of host_stage.h built in the pinned buffer and sent to c->hb_src
 * in one copy (counted in h2d_bytes); the device tables are at o_off and o_sz of c->hb_src.
 * tail_bytes: room the caller wants in the pinned buffer behind the streams, at o_tail (16-byte aligned), for a table of its own
 * that it fills and uploads in a second copy; the pinned buffer gets its final size here, before anything is queued, so it stays
 * where it is.
 * spread: the host copies go over the staging workers (recompression, whose large calls come through here too; a large
 * decompress or check call takes the pipelined staging instead) */
struct StagedStreams { size_t o_off = 0, o_sz = 0, o_data = 0, total = 0, o_tail = 0; };
static int stage_streams(cryo_codec *c, const void *const *h_src, const uint32_t *h_src_size, size_t n, StagedStreams &sg, bool spread = false, size_t tail_bytes = 0)
{
    if (!streams_ok(h_src, h_src_size, n)) return CRYO_E_ARG;
    const auto size_of = [&](size_t i) { return h_src_size[i]; };
    const cryo::StreamLayout L(n, size_of);
    sg = {L.o_off, L.o_sz, L.o_data, L.total, (L.bytes() + 64 + 15) & ~(size_t)15}; /* o_tail = bytes + 64: both are multiples of 16 */
    int rc;
    if ((rc = ensure_pinned(c, sg.o_tail + tail_bytes)) != CRYO_OK) return rc;
    if ((rc = ensure(c, &c->hb_src, &c->hb_src_cap, L.bytes() + 64)) != CRYO_OK) return rc;
    write_staged(c, L, (uint8_t *)c->pin, [&](size_t i) { return h_src[i]; }, size_of, spread);
    HIP_TRY(c, hipMemcpyAsync(c->hb_src, c->pin, L.bytes(), hipMemcpyHostToDevice, c->stream));
    c->xfer_ctr.h2d_bytes += L.bytes();
    return CRYO_OK;
}

/* Decode or check: what a staged call runs on the blocks lo .. lo+cnt of the device tables, and what comes back.  The staging
 * (staged_piped, staged_blocks) takes both from one of these two and asks no further.  p_st: the pipelined call's room for n
 * statuses in the pinned buffer */
struct CheckOp { /* only the results come back: no decoded blocks, no statuses */
    cryo_codec *c; int method; size_t block_size, n; cryo_check_result *h_result;
    cryo_check_result *d_res() const { return (cryo_check_result *)c->hb_meta; }
    size_t out_block() const { return 0; } /* the bytes per block that are decoded to come back: the staging reserves their room */
    size_t back_bytes() const { return n * sizeof(cryo_check_result); } /* what the call adds to d2h_bytes */
    /* the kernels over blocks lo .. lo+cnt, on the codec stream */
    int run(const uint64_t *d_off, const uint32_t *d_sz, size_t lo, size_t cnt)
    {
        const int rc = check_pass(c, method, c->hb_src, d_off + lo, d_sz + lo, (uint32_t)block_size, cnt, d_res() + lo);
        if (rc != CRYO_OK) (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    /* pipelined, kernels per chunk: chunk ch's uploads are queued */
    int run_chunk(const uint64_t *d_off, const uint32_t *d_sz, const cryo::ChunkCut &cut, size_t ch, int32_t *) { return run(d_off, d_sz, cut.lo(ch), cut.cnt(ch)); }
    /* every launch is queued: of the pipelined call, of the one-shot call */
    int finish_piped(const cryo::ChunkCut &, bool, int32_t *) { return finish(); }
    int finish()
    {
        HIP_TRY(c, hipMemcpyAsync(h_result, d_res(), n * sizeof(cryo_check_result), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return CRYO_OK;
    }
};
/* h_dst: one contiguous K-block buffer; or one destination per block in h_dst_each (the cache's slots, a multi-GPU share): then a
 * block that failed leaves its destination untouched -- the statuses of a chunk travel with its blocks */
struct DecodeOp {
    cryo_codec *c; int method; size_t block_size, n;
    uint8_t *h_dst; void *const *h_dst_each; int32_t *h_status;
    int32_t *d_st() const { return (int32_t *)c->hb_meta; }
    size_t out_block() const { return block_size; }
    size_t back_bytes() const { return n * block_size + n * sizeof(int32_t); }
    int run(const uint64_t *d_off, const uint32_t *d_sz, size_t lo, size_t cnt)
    {
        const int rc = cryo_codec_decompress_batch(c, method, c->hb_src, d_off + lo, d_sz + lo, c->hb_dst + lo * block_size, block_size, (uint32_t)block_size, cnt, d_st() + lo);
        if (rc != CRYO_OK) (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    /* chunk ch, once it lies in its pinned buffer, to the caller */
    int landed(const cryo::ChunkCut &cut, size_t ch, const int32_t *p_st)
    {
        const size_t lo = cut.lo(ch), cnt = cut.cnt(ch);
        const uint8_t *from = (const uint8_t *)c->pipe_pin[2 + (ch & 1)];
        HIP_TRY(c, hipEventSynchronize(c->ev_out[ch & 1]));
        if (!h_dst) return hand_back(c, p_st + lo, h_dst_each + lo, from, false, cnt, block_size);
        parallel_copy(c, {{h_dst + lo * block_size, from, cnt * block_size}});
        return CRYO_OK;
    }
    /* chunk ch leaves on the transfer stream behind its kernel, into the buffer that chunk ch-2 has been scattered from */
    int run_chunk(const uint64_t *d_off, const uint32_t *d_sz, const cryo::ChunkCut &cut, size_t ch, int32_t *p_st)
    {
        const size_t lo = cut.lo(ch), cnt = cut.cnt(ch);
        const int b = (int)(ch & 1);
        int rc = run(d_off, d_sz, lo, cnt);
        if (rc != CRYO_OK) { (void)hipStreamSynchronize(c->xfer); return rc; }
        HIP_TRY(c, hipEventRecord(c->ev_k[b], c->stream));
        if (ch >= 2 && (rc = landed(cut, ch - 2, p_st)) != CRYO_OK) return rc; /* frees output buffer b */
        HIP_TRY(c, hipStreamWaitEvent(c->xfer, c->ev_k[b], 0));
        HIP_TRY(c, hipMemcpyAsync(c->pipe_pin[2 + b], c->hb_dst + lo * block_size, cnt * block_size, hipMemcpyDeviceToHost, c->xfer));
        if (!h_dst) HIP_TRY(c, hipMemcpyAsync(p_st + lo, d_st() + lo, cnt * 4, hipMemcpyDeviceToHost, c->xfer)); /* the scatter skips failed blocks */
        HIP_TRY(c, hipEventRecord(c->ev_out[b], c->xfer));
        return CRYO_OK;
    }
    int finish_piped(const cryo::ChunkCut &cut, bool per_chunk, int32_t *p_st)
    {
        int rc = CRYO_OK;
        if (per_chunk) {
            for (size_t ch = cut.chunks() >= 2 ? cut.chunks() - 2 : 0; ch < cut.chunks() && rc == CRYO_OK; ch++) rc = landed(cut, ch, p_st);
        } else {
            HIP_TRY(c, hipEventRecord(c->ev_k[0], c->stream));
            HIP_TRY(c, hipStreamWaitEvent(c->xfer, c->ev_k[0], 0));
            if (!h_dst) HIP_TRY(c, hipMemcpyAsync(p_st, d_st(), n * 4, hipMemcpyDeviceToHost, c->xfer)); /* before the first chunk's event */
            rc = pipe_return(c, cut, c->hb_dst, block_size, [&](size_t ch) { return cut.cnt(ch) * block_size; },
                             [&](size_t ch) { return landed(cut, ch, p_st); });
        }
        if (rc != CRYO_OK) return rc;
        /* the scatters read p_st on the host (which blocks failed): the whole-call status copy goes out behind them, not under them */
        HIP_TRY(c, hipMemcpyAsync(p_st, d_st(), n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        memcpy(h_status, p_st, n * 4);
        return CRYO_OK;
    }
    /* one destination per block: the blocks come back in ONE copy into the pinned buffer (the compressed side of it is no longer
     * needed) and are handed to their destinations from there; without the room for that, block by block from the device */
    int finish()
    {
        HIP_TRY(c, hipMemcpyAsync(h_status, d_st(), n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        const bool by_pin = !h_dst && ensure_pinned(c, n * block_size) == CRYO_OK;
        if (h_dst || by_pin) HIP_TRY(c, hipMemcpyAsync(h_dst ? h_dst : c->pin, c->hb_dst, n * block_size, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (h_dst) return CRYO_OK;
        const int rc = hand_back(c, h_status, h_dst_each, by_pin ? (const uint8_t *)c->pin : c->hb_dst, !by_pin, n, block_size);
        if (rc != CRYO_OK || by_pin) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return CRYO_OK;
    }
};

/* the pipelined staging: the tables go up first, the streams chunk by chunk through the two pinned input buffers (host gather of
 * chunk c+1 under the H2D of chunk c), the kernels per chunk or once over the whole call (host_stage.h) */
template <class Op> static int staged_piped(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n, size_t block_size, Op &op)
{
    if (!streams_ok(h_src, h_src_size, n)) return CRYO_E_ARG;
    const cryo::ChunkCut cut(n, block_size);
    const bool per_chunk = cryo::kernel_per_chunk(cut.K, method == CRYO_METHOD_LZ4, false);
    const auto size_of = [&](size_t i) { return h_src_size[i]; };
    const cryo::StreamLayout L(n, size_of);
    int rc;
    if ((rc = ensure_pipe_streams(c)) != CRYO_OK) return rc;
    if ((rc = ensure_pinned(c, L.o_data + n * 4 + 64)) != CRYO_OK) return rc;
    if ((rc = ensure(c, &c->hb_src, &c->hb_src_cap, L.bytes() + 64)) != CRYO_OK) return rc;
    if (op.out_block() && (rc = ensure(c, &c->hb_dst, &c->hb_dst_cap, n * op.out_block() + 64)) != CRYO_OK) return rc;
    if ((rc = ensure(c, &c->hb_meta, &c->hb_meta_cap, n * 16 + 64)) != CRYO_OK) return rc;
    const size_t max_chunk_in = L.max_chunk_in(cut);
    for (int b = 0; b < 2; b++) {
        if ((rc = ensure_pipe(c, b, max_chunk_in + 64)) != CRYO_OK) return rc;
        if (op.out_block() && (rc = ensure_pipe(c, 2 + b, cut.K * op.out_block())) != CRYO_OK) return rc;
    }
    uint8_t *pin = (uint8_t *)c->pin;
    int32_t *p_st = (int32_t *)(pin + L.o_data);
    L.fill_tables(pin, size_of);
    HIP_TRY(c, hipMemcpyAsync(c->hb_src, pin, L.o_data, hipMemcpyHostToDevice, c->stream));
    c->xfer_ctr.h2d_bytes += L.bytes();
    c->xfer_ctr.d2h_bytes += op.back_bytes();
    const uint64_t *d_off = (const uint64_t *)(c->hb_src + L.o_off);
    const uint32_t *d_sz = (const uint32_t *)(c->hb_src + L.o_sz);
    for (size_t ch = 0; ch < cut.chunks(); ch++) {
        const size_t lo = cut.lo(ch), hi = cut.hi(ch);
        const int b = (int)(ch & 1);
        if (ch >= 2) HIP_TRY(c, hipEventSynchronize(c->ev_in[b]));
        std::vector<CopyJob> jobs;
        for (size_t i = lo; i < hi; i++)
            if (h_src_size[i]) jobs.push_back({(uint8_t *)c->pipe_pin[b] + L.span(lo, i), h_src[i], h_src_size[i]});
        parallel_copy(c, jobs);
        if (L.span(lo, hi)) HIP_TRY(c, hipMemcpyAsync(c->hb_src + L.offset(lo), c->pipe_pin[b], L.span(lo, hi), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipEventRecord(c->ev_in[b], c->stream));
        if (per_chunk && (rc = op.run_chunk(d_off, d_sz, cut, ch, p_st)) != CRYO_OK) return rc;
    }
    if (!per_chunk && (rc = op.run(d_off, d_sz, 0, n)) != CRYO_OK) return rc;
    return op.finish_piped(cut, per_chunk, p_st);
}

/* n streams given by pointer through op: pipelined when the call is large, else staged, uploaded and run in one piece.  The caller
 * has checked the arguments */
template <class Op> static int staged_blocks(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n, size_t block_size, Op op)
{
    DevGuard dev_(c);
    ScopedLocalCpus numa_(c, n, block_size);
    if (pipe_worth_it(c, n, block_size))
        return piped(c, [&] { return staged_piped(c, method, h_src, h_src_size, n, block_size, op); });
    StagedStreams sg;
    int rc;
    /* every allocation of the call before the upload is queued and counted */
    if (op.out_block() && (rc = ensure(c, &c->hb_dst, &c->hb_dst_cap, n * op.out_block() + 64)) != CRYO_OK) return rc;
    if ((rc = ensure(c, &c->hb_meta, &c->hb_meta_cap, n * 16 + 64)) != CRYO_OK) return rc;
    if ((rc = stage_streams(c, h_src, h_src_size, n, sg)) != CRYO_OK) return rc;
    c->xfer_ctr.d2h_bytes += op.back_bytes();
    if ((rc = op.run((const uint64_t *)(c->hb_src + sg.o_off), (const uint32_t *)(c->hb_src + sg.o_sz), 0, n)) != CRYO_OK) return rc;
    return op.finish();
}

static int decompress_blocks_host(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                                  void *h_dst, void *const *h_dst_each, size_t block_size, int32_t *h_status)
{
    if (!c || !method_ok(method) || !block_size_ok(block_size)) return CRYO_E_ARG;
    if (n == 0) return CRYO_OK;
    if (!h_src || !h_src_size || (!h_dst && !h_dst_each) || !h_status) return CRYO_E_ARG;
    return staged_blocks(c, method, h_src, h_src_size, n, block_size, DecodeOp{c, method, block_size, n, (uint8_t *)h_dst, h_dst_each, h_status});
}

extern "C" {

int cryo_codec_compress_blocks(cryo_codec *c, int method, int param, const void *h_src, size_t block_size,
                               size_t n, void *h_dst, size_t dst_stride, uint32_t *h_out_size)
{
    return host_call(c, [&]() -> int {
        if (!c || !method_ok(method) || !block_size_ok(block_size)) return CRYO_E_ARG;
        if (n == 0) return CRYO_OK;
        if (!h_src || !h_dst || !h_out_size) return CRYO_E_ARG;
        if (dst_stride < cryo_codec_bound(method, block_size)) return CRYO_E_DSTSIZE;
        return compress_blocks_host(c, method, param, {(const uint8_t *)h_src, (uint8_t *)h_dst, dst_stride, nullptr, nullptr}, block_size, n, h_out_size);
    });
}

int cryo_codec_decompress_blocks(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size,
                                 size_t n, void *h_dst, size_t block_size, int32_t *h_status)
{
    if (!h_dst) return CRYO_E_ARG;
    return host_call(c, [&] {
        return decompress_blocks_host(c, method, h_src, h_src_size, n, h_dst, nullptr, block_size, h_status);
    });
}

int cryo_codec_decompress_blocks_to(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size,
                                    size_t n, void *const *h_dst, size_t block_size, int32_t *h_status)
{
    if (!h_dst) return CRYO_E_ARG;
    return host_call(c, [&] {
        return decompress_blocks_host(c, method, h_src, h_src_size, n, nullptr, h_dst, block_size, h_status);
    });
}

int cryo_codec_check_blocks(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                            size_t block_size, cryo_check_result *h_result)
{
    if (!c || !method_ok(method) || !check_block_size_ok(block_size)) return CRYO_E_ARG;
    if (n == 0) return CRYO_OK;
    if (!h_src || !h_src_size || !h_result) return CRYO_E_ARG;
    return host_call(c, [&] { return staged_blocks(c, method, h_src, h_src_size, n, block_size, CheckOp{c, method, block_size, n, h_result}); });
}

/* recompression of n streams given by pointer: staged and uploaded as the stored-block check's (stage_streams), recoded chunk
 * by chunk on the device, and only the packed streams, the sizes and the statuses come back.  h_base: what the call's offsets
 * count from (a multi-GPU share's region within the caller's h_dst) */
static int recode_blocks_impl(cryo_codec *c, int src_method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                              size_t block_size, int dst_method, int dst_param, void *h_dst, size_t dst_cap, uint64_t h_base,
                              uint64_t *h_out_off, uint32_t *h_out_size, int32_t *h_status)
{
    DevGuard dev_(c);
    const int ok = recode_args(c, src_method, dst_method, dst_param, block_size);
    if (ok != CRYO_OK) return ok;
    if (n == 0) return CRYO_OK;
    if (!h_src || !h_src_size || !h_dst || !h_out_off || !h_out_size || !h_status) return CRYO_E_ARG;
    ScopedLocalCpus numa_(c, n, block_size);
    StagedStreams sg;
    int rc;
    if ((rc = stage_streams(c, h_src, h_src_size, n, sg, true)) != CRYO_OK) return rc;
    const size_t o_off = sg.o_off, o_sz = sg.o_sz;
    RecodeOut out;
    out.h_dst = (uint8_t *)h_dst; out.dst_cap = dst_cap; out.h_base = h_base;
    out.h_off = h_out_off; out.h_size = h_out_size; out.h_status = h_status;
    rc = recode_pass(c, src_method, c->hb_src, (const uint64_t *)(c->hb_src + o_off), (const uint32_t *)(c->hb_src + o_sz),
                     (uint32_t)block_size, n, dst_method, dst_param, out);
    if (rc != CRYO_OK) (void)hipStreamSynchronize(c->stream); /* nothing in flight into the caller's memory after an error */
    return rc;
}

int cryo_codec_recode_blocks(cryo_codec *c, int src_method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                             size_t block_size, int dst_method, int dst_param, void *h_dst, size_t dst_cap, uint64_t *h_out_off,
                             uint32_t *h_out_size, int32_t *h_status)
{
    return host_call(c, [&] {
        return recode_blocks_impl(c, src_method, h_src, h_src_size, n, block_size, dst_method, dst_param, h_dst, dst_cap, 0,
                                          h_out_off, h_out_size, h_status);
    });
}

/* the tuple fetch of n streams given by pointer: the streams staged and uploaded as recompression's (stage_streams), the request
 * table from the same pinned buffer in a second copy, both into place before the first decode; records and tuples come back
 * chunk by chunk (fetch_pass).  h_base: what the records' offsets count from (a multi-GPU share's region within the caller's
 * h_dst); *h_total is relative to h_dst as given here */
static int fetch_blocks_impl(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                             size_t block_size, const uint64_t *h_req_first, const uint16_t *h_pos, void *h_dst, size_t dst_cap,
                             uint64_t h_base, cryo_fetch_result *h_result, uint64_t *h_total)
{
    DevGuard dev_(c);
    if (!c || !method_ok(method) || !check_block_size_ok(block_size) || !h_total) return CRYO_E_ARG;
    *h_total = 0;
    if (n == 0) return CRYO_OK;
    if (!h_src || !h_src_size || !h_req_first || h_req_first[0] != 0) return CRYO_E_ARG;
    for (size_t i = 0; i < n; i++)
        if (h_req_first[i + 1] < h_req_first[i]) return CRYO_E_ARG;
    const uint64_t n_req = h_req_first[n];
    if (n_req > 0 && (!h_pos || !h_result)) return CRYO_E_ARG;
    if (!h_dst && dst_cap > 0) return CRYO_E_ARG;
    ScopedLocalCpus numa_(c, n, block_size);
    /* the request table: [first u64 x (n + 1)][pos u16 x n_req][records x n_req], each part 16-byte aligned */
    const size_t t_first = 0, t_pos = ((n + 1) * 8 + 15) & ~(size_t)15, t_rec = t_pos + ((n_req * 2 + 15) & ~(size_t)15);
    int rc;
    /* every allocation of the call before the uploads are queued; the table goes into the tail behind the staged streams */
    if ((rc = ensure(c, &c->hb_meta, &c->hb_meta_cap, t_rec + n_req * sizeof(cryo_fetch_result) + 64)) != CRYO_OK) return rc;
    StagedStreams sg;
    if ((rc = stage_streams(c, h_src, h_src_size, n, sg, true, t_rec)) != CRYO_OK) return rc;
    uint8_t *pin = (uint8_t *)c->pin + sg.o_tail;
    memset(pin, 0, t_rec);
    memcpy(pin + t_first, h_req_first, (n + 1) * 8);
    if (n_req) memcpy(pin + t_pos, h_pos, n_req * 2);
    HIP_TRY(c, hipMemcpyAsync(c->hb_meta, pin, t_rec, hipMemcpyHostToDevice, c->stream));
    c->xfer_ctr.h2d_bytes += t_rec;
    FetchIo io;
    io.d_req_first = (const uint64_t *)(c->hb_meta + t_first); io.d_pos = (const uint16_t *)(c->hb_meta + t_pos);
    io.n_req = n_req; io.d_result = (cryo_fetch_result *)(c->hb_meta + t_rec);
    io.h_req_first = h_req_first; io.h_dst = (uint8_t *)h_dst; io.dst_cap = dst_cap; io.h_result = h_result;
    rc = fetch_pass(c, method, c->hb_src, (const uint64_t *)(c->hb_src + sg.o_off), (const uint32_t *)(c->hb_src + sg.o_sz),
                    (uint32_t)block_size, n, io);
    (void)hipStreamSynchronize(c->stream); /* nothing in flight from the pinned buffer or into the caller's memory */
    if (rc != CRYO_OK) return rc;
    if (h_base)
        for (uint64_t r = 0; r < n_req; r++) h_result[r].off += h_base;
    *h_total = io.h_total;
    return CRYO_OK;
}

int cryo_codec_fetch_blocks(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                            size_t block_size, const uint64_t *h_req_first, const uint16_t *h_pos, void *h_dst, size_t dst_cap,
                            cryo_fetch_result *h_result, uint64_t *h_total)
{
    return host_call(c, [&] {
        return fetch_blocks_impl(c, method, h_src, h_src_size, n, block_size, h_req_first, h_pos, h_dst, dst_cap, 0, h_result,
                                         h_total);
    });
}

/* The descriptor of a host-buffer scan call: [atts 4 x natts][keys 16 x nkeys][byte-string constants][the call's extra bytes:
 * the aggregate's columns, the group's six slots], each part 16-byte aligned.  It takes the first `bytes` of c->hb_meta, where
 * the call's results follow it */
struct ScanDescLayout { size_t t_keys = 0, t_extra = 0, bytes = 0; bool table_keys = false, floats = false, like = false; };
/* cols: the call's ncols aggregate columns, where it has some */
static ScanDescLayout scan_desc_layout(const cryo_filter *f, size_t extra_bytes, const cryo_agg_col *cols = nullptr, uint32_t ncols = 0)
{
    ScanDescLayout L;
    L.floats = desc_has_float(f->keys, f->nkeys, cols, ncols);
    L.like = desc_has_like(f->keys, f->nkeys);
    L.t_keys = ((size_t)f->natts * 4 + 15) & ~(size_t)15;
    L.t_extra = L.t_keys + (size_t)f->nkeys * 16 + key_consts_bytes(f->keys, f->nkeys, &L.table_keys);
    L.bytes = L.t_extra + extra_bytes;
    return L;
}
/* stages the streams (stage_streams) with the descriptor in the tail behind them, uploads it in a second copy (counted in
 * h2d_bytes), both into place before the first decode, and fills sd.  c->hb_meta holds L.bytes and the call's results already:
 * every allocation of the call is made before the uploads are queued.  extra: the call's extra bytes, zero-padded */
static int scan_desc_upload(cryo_codec *c, const void *const *h_src, const uint32_t *h_src_size, size_t n, const cryo_filter *f,
                            uint32_t max_att, const ScanDescLayout &L, const void *extra, StagedStreams &sg, ScanDesc &sd)
{
    const int rc = stage_streams(c, h_src, h_src_size, n, sg, true, L.bytes);
    if (rc != CRYO_OK) return rc;
    uint8_t *pin = (uint8_t *)c->pin + sg.o_tail;
    memset(pin, 0, L.bytes);
    memcpy(pin, f->atts, (size_t)f->natts * 4);
    if (!key_table_host(pin + L.t_keys, c->hb_meta + L.t_keys, f)) return CRYO_E_ARG;
    if (L.bytes > L.t_extra) memcpy(pin + L.t_extra, extra, L.bytes - L.t_extra);
    HIP_TRY(c, hipMemcpyAsync(c->hb_meta, pin, L.bytes, hipMemcpyHostToDevice, c->stream));
    c->xfer_ctr.h2d_bytes += L.bytes;
    sd.d_atts = c->hb_meta; sd.d_keys = c->hb_meta + L.t_keys; sd.nkeys = f->nkeys; sd.max_att = max_att; sd.floats = L.floats; sd.like = L.like; sd.truth = scan_truth(f, L.table_keys || L.floats);
    return CRYO_OK;
}

/* what every host-buffer filter call checks before a device is touched */
static int filter_blocks_args(int method, size_t block_size, const cryo_filter *f, uint64_t *h_total, uint32_t *max_att)
{
    if (!method_ok(method) || !check_block_size_ok(block_size) || !h_total) return CRYO_E_ARG;
    if (!f || !filter_desc_ok(f, f->atts, f->keys, max_att)) return CRYO_E_ARG;
    return CRYO_OK;
}

/* the scan filter of n streams given by pointer: the streams staged and uploaded as the fetch's (stage_streams), the descriptor
 * from the same pinned buffer in a second copy, both into place before the first decode; table, records and tuples come back
 * chunk by chunk (filter_pass).  b_base / r_base: what the table's `off` / rec_first count from (a multi-GPU share's regions
 * within the caller's buffers); h_total is relative to h_dst / h_rec as given here */
static int filter_blocks_impl(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                              size_t block_size, const cryo_filter *f, void *h_dst, size_t dst_cap, uint64_t b_base,
                              cryo_filter_rec *h_rec, size_t rec_cap, uint64_t r_base, cryo_filter_block *h_blocks, uint64_t *h_total)
{
    uint32_t max_att = 0;
    int rc = filter_blocks_args(method, block_size, f, h_total, &max_att);
    if (rc != CRYO_OK || !c) return CRYO_E_ARG;
    DevGuard dev_(c);
    h_total[0] = h_total[1] = 0;
    if (n == 0) return CRYO_OK;
    const bool count_only = (f->flags & CRYO_FILTER_COUNT_ONLY) != 0;
    if (!h_src || !h_src_size || !h_blocks) return CRYO_E_ARG;
    if (!count_only && ((!h_dst && dst_cap > 0) || (!h_rec && rec_cap > 0))) return CRYO_E_ARG;
    ScopedLocalCpus numa_(c, n, block_size);
    /* the descriptor, then the table: [rows 32 x n] */
    const ScanDescLayout L = scan_desc_layout(f, 0);
    const size_t t_rows = L.bytes;
    if ((rc = ensure(c, &c->hb_meta, &c->hb_meta_cap, t_rows + n * sizeof(cryo_filter_block) + 64)) != CRYO_OK) return rc;
    StagedStreams sg;
    FilterIo io;
    if ((rc = scan_desc_upload(c, h_src, h_src_size, n, f, max_att, L, nullptr, sg, io.sd)) != CRYO_OK) return rc;
    io.count_only = count_only; io.d_blocks = (cryo_filter_block *)(c->hb_meta + t_rows);
    io.dst_cap = count_only ? 0 : dst_cap; io.rec_cap = count_only ? 0 : rec_cap;
    io.host = true; io.h_blocks = h_blocks; io.h_rec = h_rec; io.h_dst = (uint8_t *)h_dst;
    rc = filter_pass(c, method, c->hb_src, (const uint64_t *)(c->hb_src + sg.o_off), (const uint32_t *)(c->hb_src + sg.o_sz),
                     (uint32_t)block_size, n, io);
    (void)hipStreamSynchronize(c->stream); /* nothing in flight from the pinned buffer or into the caller's memory */
    if (rc != CRYO_OK) return rc;
    if (!count_only && (b_base || r_base))
        for (size_t i = 0; i < n; i++) { h_blocks[i].off += b_base; h_blocks[i].rec_first += r_base; }
    h_total[0] = io.h_bytes;
    h_total[1] = io.h_recs;
    return CRYO_OK;
}

int cryo_codec_filter_blocks(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                             size_t block_size, const cryo_filter *f, void *h_dst, size_t dst_cap, cryo_filter_rec *h_rec,
                             size_t rec_cap, cryo_filter_block *h_blocks, uint64_t *h_total)
{
    return host_call(c, [&] {
        return filter_blocks_impl(c, method, h_src, h_src_size, n, block_size, f, h_dst, dst_cap, 0, h_rec, rec_cap, 0,
                                          h_blocks, h_total);
    });
}

/* what every host-buffer aggregate call checks before a device is touched */
static int agg_blocks_args(int method, size_t block_size, const cryo_filter *f, const cryo_agg *agg, uint32_t *max_att)
{
    if (!method_ok(method) || !check_block_size_ok(block_size)) return CRYO_E_ARG;
    if (!f || !agg || !agg_desc_ok(f, f->atts, f->keys, agg, agg->cols, max_att)) return CRYO_E_ARG;
    return CRYO_OK;
}

/* the readback of a host-buffer scan call: after a pass that went well, up to two device-to-host copies (one of no bytes is left
 * out), counted in d2h_bytes when they were queued; then, whatever rc says, the wait for the stream -- nothing in flight from the
 * pinned buffer or into the caller's memory afterwards.  The first error is the call's; `what` names the copies for it */
struct Readback { void *dst; const void *src; size_t bytes; };
static int read_back(cryo_codec *c, int rc, const Readback &a, const Readback &b, const char *what)
{
    if (rc == CRYO_OK) {
        hipError_t e = hipMemcpyAsync(a.dst, a.src, a.bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && b.bytes) e = hipMemcpyAsync(b.dst, b.src, b.bytes, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) rc = fail(c, e, what);
        else c->xfer_ctr.d2h_bytes += a.bytes + b.bytes;
    }
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (rc == CRYO_OK && es != hipSuccess) rc = fail(c, es, "hipStreamSynchronize");
    return rc;
}

/* the scan aggregate of n streams given by pointer: the streams staged and uploaded as the filter's (stage_streams), the
 * descriptors from the same pinned buffer in a second copy, both into place before the first decode; rows and cells of the whole
 * call come back after the last chunk (agg_pass waits for nothing) */
static int agg_blocks_impl(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                           size_t block_size, const cryo_filter *f, const cryo_agg *agg, cryo_agg_block *h_blocks,
                           cryo_agg_cell *h_cells)
{
    uint32_t max_att = 0;
    int rc = agg_blocks_args(method, block_size, f, agg, &max_att);
    if (rc != CRYO_OK || !c) return CRYO_E_ARG;
    DevGuard dev_(c);
    if (n == 0) return CRYO_OK;
    if (!h_src || !h_src_size || !h_blocks || !h_cells) return CRYO_E_ARG;
    ScopedLocalCpus numa_(c, n, block_size);
    /* the descriptor with [cols 8 x ncols] as its extra bytes, then the results: [rows 16 x n][cells 40 x n x ncols] */
    cryo_agg_col cols[CRYO_AGG_MAX_COLS] = {};
    memcpy(cols, agg->cols, (size_t)agg->ncols * 8);
    const ScanDescLayout L = scan_desc_layout(f, ((size_t)agg->ncols * 8 + 15) & ~(size_t)15, cols, agg->ncols);
    const size_t t_rows = L.bytes;
    const size_t rows_bytes = n * sizeof(cryo_agg_block), cells_bytes = n * agg->ncols * sizeof(cryo_agg_cell);
    if ((rc = ensure(c, &c->hb_meta, &c->hb_meta_cap, t_rows + rows_bytes + cells_bytes + 64)) != CRYO_OK) return rc;
    StagedStreams sg;
    AggIo io;
    if ((rc = scan_desc_upload(c, h_src, h_src_size, n, f, max_att, L, cols, sg, io.sd)) != CRYO_OK) return rc;
    io.d_cols = c->hb_meta + L.t_extra; io.ncols = agg->ncols;
    io.d_blocks = (cryo_agg_block *)(c->hb_meta + t_rows);
    io.d_cells = (cryo_agg_cell *)(c->hb_meta + t_rows + rows_bytes);
    rc = agg_pass(c, method, c->hb_src, (const uint64_t *)(c->hb_src + sg.o_off), (const uint32_t *)(c->hb_src + sg.o_sz),
                  (uint32_t)block_size, n, io);
    /* the call's one wait */
    return read_back(c, rc, {h_blocks, io.d_blocks, rows_bytes}, {h_cells, io.d_cells, cells_bytes}, "hipMemcpyAsync of rows and cells");
}

int cryo_codec_agg_blocks(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                          size_t block_size, const cryo_filter *f, const cryo_agg *agg, cryo_agg_block *h_blocks,
                          cryo_agg_cell *h_cells)
{
    return host_call(c, [&] { return agg_blocks_impl(c, method, h_src, h_src_size, n, block_size, f, agg, h_blocks, h_cells); });
}

/* what every host-buffer group call checks before a device is touched */
static int group_blocks_args(int method, size_t block_size, const cryo_filter *f, const cryo_group *grp, const cryo_agg *agg,
                             uint64_t *h_total, uint32_t *max_att, uint32_t *ncols, uint32_t *text)
{
    if (!method_ok(method) || !check_block_size_ok(block_size) || !h_total) return CRYO_E_ARG;
    if (!f || !grp || !group_desc_ok(f, f->atts, f->keys, grp, grp->by, group_buckets(grp), agg, agg ? agg->cols : nullptr, max_att, ncols, text))
        return CRYO_E_ARG;
    return CRYO_OK;
}

/* the grouped scan of n streams given by pointer: the streams staged and uploaded as the aggregate's (stage_streams), the
 * descriptors -- the two column arrays as the kernel's six slots -- from the same pinned buffer in a second copy, both into place
 * before the first decode; the rows of the whole call come back after the last chunk (group_pass waits for nothing), then -- their
 * number known from the last row -- its records and cells */
static int group_blocks_impl(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                             size_t block_size, const cryo_filter *f, const cryo_group *grp, const cryo_agg *agg,
                             cryo_group_block *h_blocks, cryo_group_rec *h_groups, size_t group_cap, cryo_agg_cell *h_cells,
                             uint64_t *h_total)
{
    uint32_t max_att = 0, ncols = 0, text = 0;
    int rc = group_blocks_args(method, block_size, f, grp, agg, h_total, &max_att, &ncols, &text);
    if (rc != CRYO_OK || !c) return CRYO_E_ARG;
    const uint32_t cpg = ncols + (uint32_t)__builtin_popcount(text); /* a group's cells: the aggregate cells, then the key cells */
    DevGuard dev_(c);
    *h_total = 0;
    if (n == 0) return CRYO_OK;
    if (!h_src || !h_src_size || !h_blocks || (group_cap > 0 && (!h_groups || (cpg > 0 && !h_cells)))) return CRYO_E_ARG;
    ScopedLocalCpus numa_(c, n, block_size);
    /* the descriptor with the kernel's six slots [by 8 x 2][cols 8 x 4] and -- CRYO_GROUP_BUCKETS -- the bucket table (built for
     * the address it will have in c->hb_meta, from the caller's host lists) as its extra bytes, then the results: [total 16]
     * [rows 32 x n][records 24 x cap][cells 40 x cap x cpg], each part 8-byte aligned, the rows 16; cap: what the caller has room
     * for, at most the worst case */
    const size_t worst = n * (size_t)cryo::filter_side_stride((uint32_t)block_size);
    const size_t cap = group_cap < worst ? group_cap : worst;
    const cryo_bucket *bk = group_buckets(grp);
    constexpr size_t kSlots = CRYO_GROUP_MAX_BY + CRYO_AGG_MAX_COLS;
    std::vector<uint64_t> extra(kSlots + (bk ? bucket_table_bytes(bk, grp->nby) / 8 : 0), 0); /* 8-byte aligned, zeroed */
    cryo_agg_col *slots = (cryo_agg_col *)extra.data();
    static_assert(sizeof(cryo_agg_col) == 8, "a slot is a word of the extra bytes");
    memcpy(slots, grp->by, (size_t)grp->nby * 8);
    if (ncols) memcpy(slots + CRYO_GROUP_MAX_BY, agg->cols, (size_t)ncols * 8);
    ScanDescLayout L = scan_desc_layout(f, extra.size() * 8, slots + CRYO_GROUP_MAX_BY, ncols);
    if (bk || text) L.table_keys = true; /* the bucket and the text kernels have the table's verdict path alone */
    const size_t t_total = L.bytes, t_rows = t_total + 16;
    const size_t rows_bytes = n * sizeof(cryo_group_block), t_recs = t_rows + rows_bytes, t_cells = t_recs + cap * sizeof(cryo_group_rec);
    if ((rc = ensure(c, &c->hb_meta, &c->hb_meta_cap, t_cells + cap * cpg * sizeof(cryo_agg_cell) + 64)) != CRYO_OK) return rc;
    StagedStreams sg;
    GroupIo io;
    if (bk) {
        const void *lists[CRYO_GROUP_MAX_BY] = {nullptr, nullptr};
        for (uint32_t j = 0; j < grp->nby; j++) lists[j] = (const void *)(uintptr_t)bk[j].value;
        uint8_t *d_tab = c->hb_meta + L.t_extra + kSlots * 8;
        bucket_table_fill((uint8_t *)(extra.data() + kSlots), (uint64_t)(uintptr_t)d_tab, bk, grp->nby, lists);
        io.sd.d_buckets = d_tab;
    }
    if ((rc = scan_desc_upload(c, h_src, h_src_size, n, f, max_att, L, extra.data(), sg, io.sd)) != CRYO_OK) return rc;
    io.d_slots = c->hb_meta + L.t_extra; io.nby = grp->nby; io.ncols = ncols; io.sd.text = text;
    io.d_total = (uint64_t *)(c->hb_meta + t_total);
    io.d_blocks = (cryo_group_block *)(c->hb_meta + t_rows);
    io.d_groups = (cryo_group_rec *)(c->hb_meta + t_recs);
    io.d_cells = (cryo_agg_cell *)(c->hb_meta + t_cells);
    io.group_cap = cap;
    rc = group_pass(c, method, c->hb_src, (const uint64_t *)(c->hb_src + sg.o_off), (const uint32_t *)(c->hb_src + sg.o_sz),
                    (uint32_t)block_size, n, io);
    rc = read_back(c, rc, {h_blocks, io.d_blocks, rows_bytes}, {}, "hipMemcpyAsync of rows");
    if (rc != CRYO_OK) return rc;
    const cryo_group_block &last = h_blocks[n - 1];
    if (last.first_group > worst || last.n_groups > worst - last.first_group) return CRYO_E_HIP; /* not a placement */
    const uint64_t total = last.first_group + last.n_groups;
    *h_total = total;
    if (total > group_cap) return CRYO_E_DSTSIZE;
    if (total)
        rc = read_back(c, rc, {h_groups, io.d_groups, total * sizeof(cryo_group_rec)},
                       {h_cells, io.d_cells, total * cpg * sizeof(cryo_agg_cell)}, "hipMemcpyAsync of records and cells");
    return rc;
}

int cryo_codec_group_blocks(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                            size_t block_size, const cryo_filter *f, const cryo_group *grp, const cryo_agg *agg,
                            cryo_group_block *h_blocks, cryo_group_rec *h_groups, size_t group_cap, cryo_agg_cell *h_cells,
                            uint64_t *h_total)
{
    return host_call(c, [&] {
        return group_blocks_impl(c, method, h_src, h_src_size, n, block_size, f, grp, agg, h_blocks, h_groups, group_cap,
                                         h_cells, h_total);
    });
}

/* what every host-buffer project call checks before a device is touched */
static int project_blocks_args(int method, size_t block_size, const cryo_filter *f, const cryo_project *prj, uint64_t *h_total,
                               uint32_t *max_att, ProjectTab *pt)
{
    if (!method_ok(method) || !check_block_size_ok(block_size) || !h_total) return CRYO_E_ARG;
    if (!f || !prj || !project_desc_ok(f, f->atts, f->keys, prj, prj->cols, max_att, pt)) return CRYO_E_ARG;
    return CRYO_OK;
}

/* the projecting scan of n streams given by pointer: the streams staged and uploaded as the aggregate's (stage_streams), the
 * descriptors -- the columns as the kernel's table -- from the same pinned buffer in a second copy, both into place before the
 * first decode; the block table of the whole call comes back after the last chunk (project_pass waits for nothing here), then --
 * their numbers known from the last row -- its records and rows.  w_base / r_base: what row_first / rec_first count from (a
 * multi-GPU share's regions within the caller's buffers); h_total is relative to h_rows / h_rec as given here */
static int project_blocks_impl(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                               size_t block_size, const cryo_filter *f, const cryo_project *prj, void *h_rows, size_t row_cap,
                               uint64_t w_base, cryo_project_rec *h_rec, size_t rec_cap, uint64_t r_base,
                               cryo_project_block *h_blocks, uint64_t *h_total)
{
    uint32_t max_att = 0;
    ProjectIo io;
    int rc = project_blocks_args(method, block_size, f, prj, h_total, &max_att, &io.pt);
    if (rc != CRYO_OK || !c) return CRYO_E_ARG;
    DevGuard dev_(c);
    h_total[0] = h_total[1] = 0;
    if (n == 0) return CRYO_OK;
    if (!h_src || !h_src_size || !h_blocks || (!h_rows && row_cap > 0) || (!h_rec && rec_cap > 0)) return CRYO_E_ARG;
    ScopedLocalCpus numa_(c, n, block_size);
    /* the descriptor with the column table [8 x ncols] as its extra bytes, then the results: [totals 16][table 32 x n]
     * [records 8 x cap_r][rows row_bytes x cap_w], each part 8-byte aligned, the table 16; the caps: what the caller has room for, at
     * most the worst case */
    const size_t worst = n * (size_t)cryo::filter_side_stride((uint32_t)block_size), rb = io.pt.row_bytes;
    const size_t cap_w = row_cap < worst ? row_cap : worst, cap_r = rec_cap < worst ? rec_cap : worst;
    const ScanDescLayout L = scan_desc_layout(f, ((size_t)io.pt.ncols * 8 + 15) & ~(size_t)15);
    const size_t t_total = L.bytes, t_table = t_total + 16, table_bytes = n * sizeof(cryo_project_block);
    const size_t t_recs = t_table + table_bytes, t_rows = t_recs + cap_r * sizeof(cryo_project_rec);
    if ((rc = ensure(c, &c->hb_meta, &c->hb_meta_cap, t_rows + cap_w * rb + 64)) != CRYO_OK) return rc;
    StagedStreams sg;
    if ((rc = scan_desc_upload(c, h_src, h_src_size, n, f, max_att, L, io.pt.tab, sg, io.sd)) != CRYO_OK) return rc;
    io.d_tab = c->hb_meta + L.t_extra;
    io.d_total = (uint64_t *)(c->hb_meta + t_total);
    io.d_blocks = (cryo_project_block *)(c->hb_meta + t_table);
    io.d_rec = (cryo_project_rec *)(c->hb_meta + t_recs);
    io.d_rows = c->hb_meta + t_rows;
    io.rec_cap = cap_r; io.row_cap = cap_w;
    rc = project_pass(c, method, c->hb_src, (const uint64_t *)(c->hb_src + sg.o_off), (const uint32_t *)(c->hb_src + sg.o_sz),
                      (uint32_t)block_size, n, io);
    rc = read_back(c, rc, {h_blocks, io.d_blocks, table_bytes}, {}, "hipMemcpyAsync of the block table");
    if (rc != CRYO_OK) return rc;
    const cryo_project_block &last = h_blocks[n - 1];
    const uint64_t last_recs = (uint64_t)last.n_match + last.n_bad;
    if (last.row_first > worst || last.n_match > worst - last.row_first || last.rec_first > worst || last_recs > worst - last.rec_first)
        return CRYO_E_HIP; /* not a placement */
    const uint64_t rows = last.row_first + last.n_match, recs = last.rec_first + last_recs;
    h_total[0] = rows;
    h_total[1] = recs;
    if (rows > row_cap || recs > rec_cap) return CRYO_E_DSTSIZE;
    if (recs)
        rc = read_back(c, rc, {h_rec, io.d_rec, recs * sizeof(cryo_project_rec)}, {h_rows, io.d_rows, rows * rb},
                       "hipMemcpyAsync of records and rows");
    if (rc == CRYO_OK && (w_base || r_base))
        for (size_t i = 0; i < n; i++) { h_blocks[i].row_first += w_base; h_blocks[i].rec_first += r_base; }
    return rc;
}

int cryo_codec_project_blocks(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                              size_t block_size, const cryo_filter *f, const cryo_project *prj, void *h_rows, size_t row_cap,
                              cryo_project_rec *h_rec, size_t rec_cap, cryo_project_block *h_blocks, uint64_t *h_total)
{
    return host_call(c, [&] {
        return project_blocks_impl(c, method, h_src, h_src_size, n, block_size, f, prj, h_rows, row_cap, 0, h_rec, rec_cap, 0, h_blocks,
                                   h_total);
    });
}

/* what every host-buffer ordered-scan call checks before a device is touched */
static int topn_blocks_args(int method, size_t block_size, const cryo_filter *f, const cryo_order *ord, const cryo_project *prj,
                            uint64_t *h_total, uint32_t *max_att, TopnTab *tt)
{
    if (!method_ok(method) || !check_block_size_ok(block_size) || !h_total) return CRYO_E_ARG;
    if (!f || !ord || !prj || ((uintptr_t)ord->by & 7u) != 0 || !topn_desc_ok(f, f->atts, f->keys, ord, ord->by, prj, prj->cols, max_att, tt))
        return CRYO_E_ARG;
    return CRYO_OK;
}

/* the ordered scan of n streams given by pointer: the streams staged and uploaded as the projection's (stage_streams), the
 * descriptors -- the order columns and the projected columns as the kernel's table -- from the same pinned buffer in a second copy,
 * both into place before the first decode; the block table of the whole call comes back after the last chunk (topn_pass waits for
 * nothing here), then -- their number known from the last row -- its records and rows.  w_base: what row_first counts from (a
 * multi-GPU share's region within the caller's buffers); *h_total is relative to h_rows / h_rec as given here */
static int topn_blocks_impl(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n, size_t block_size,
                            const cryo_filter *f, const cryo_order *ord, const cryo_project *prj, void *h_rows, cryo_topn_rec *h_rec,
                            size_t row_cap, uint64_t w_base, cryo_topn_block *h_blocks, uint64_t *h_total)
{
    uint32_t max_att = 0;
    TopnIo io;
    int rc = topn_blocks_args(method, block_size, f, ord, prj, h_total, &max_att, &io.tt);
    if (rc != CRYO_OK || !c) return CRYO_E_ARG;
    DevGuard dev_(c);
    *h_total = 0;
    if (n == 0) return CRYO_OK;
    if (!h_src || !h_src_size || !h_blocks || ((!h_rows || !h_rec) && row_cap > 0)) return CRYO_E_ARG;
    ScopedLocalCpus numa_(c, n, block_size);
    /* the descriptor with the kernel's table [8 x 10] as its extra bytes, then the results: [total 16][table 32 x n]
     * [records 24 x cap][rows row_bytes x cap], each part 8-byte aligned, the table 16; cap: what the caller has room for, at most
     * the worst case */
    const size_t worst = n * (size_t)topn_per_block(io.tt.limit, cryo::filter_side_stride((uint32_t)block_size)), rb = io.tt.row_bytes;
    const size_t cap = row_cap < worst ? row_cap : worst;
    const ScanDescLayout L = scan_desc_layout(f, (sizeof io.tt.slots + 15) & ~(size_t)15);
    const size_t t_total = L.bytes, t_table = t_total + 16, table_bytes = n * sizeof(cryo_topn_block);
    const size_t t_recs = t_table + table_bytes, t_rows = t_recs + cap * sizeof(cryo_topn_rec);
    if ((rc = ensure(c, &c->hb_meta, &c->hb_meta_cap, t_rows + cap * rb + 64)) != CRYO_OK) return rc;
    StagedStreams sg;
    if ((rc = scan_desc_upload(c, h_src, h_src_size, n, f, max_att, L, io.tt.slots, sg, io.sd)) != CRYO_OK) return rc;
    io.d_tab = c->hb_meta + L.t_extra;
    io.d_total = (uint64_t *)(c->hb_meta + t_total);
    io.d_blocks = (cryo_topn_block *)(c->hb_meta + t_table);
    io.d_rec = (cryo_topn_rec *)(c->hb_meta + t_recs);
    io.d_rows = c->hb_meta + t_rows;
    io.row_cap = cap;
    rc = topn_pass(c, method, c->hb_src, (const uint64_t *)(c->hb_src + sg.o_off), (const uint32_t *)(c->hb_src + sg.o_sz),
                   (uint32_t)block_size, n, io);
    rc = read_back(c, rc, {h_blocks, io.d_blocks, table_bytes}, {}, "hipMemcpyAsync of the block table");
    if (rc != CRYO_OK) return rc;
    const cryo_topn_block &last = h_blocks[n - 1];
    if (last.row_first > worst || last.n_rows > worst - last.row_first) return CRYO_E_HIP; /* not a placement */
    const uint64_t rows = last.row_first + last.n_rows;
    *h_total = rows;
    if (rows > row_cap) return CRYO_E_DSTSIZE;
    if (rows)
        rc = read_back(c, rc, {h_rec, io.d_rec, rows * sizeof(cryo_topn_rec)}, {h_rows, io.d_rows, rows * rb}, "hipMemcpyAsync of records and rows");
    if (rc == CRYO_OK && w_base)
        for (size_t i = 0; i < n; i++) h_blocks[i].row_first += w_base;
    return rc;
}

int cryo_codec_topn_blocks(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n, size_t block_size,
                           const cryo_filter *f, const cryo_order *ord, const cryo_project *prj, void *h_rows, cryo_topn_rec *h_rec,
                           size_t row_cap, cryo_topn_block *h_blocks, uint64_t *h_total)
{
    return host_call(c, [&] {
        return topn_blocks_impl(c, method, h_src, h_src_size, n, block_size, f, ord, prj, h_rows, h_rec, row_cap, 0, h_blocks, h_total);
    });
}

} /* extern "C" */

/* ---- device-resident block pool ---- */
/* Identity of a compressed stream in the pool: a 64-bit hash of ALL its bytes (four multiply-rotate lanes, 32 bytes per
 * step, about 10 GB/s on one host core -- next to nothing beside the transfer and the decode a hit saves).  Round 3
 * sampled 24 bytes (first, middle, last 8): a rewritten block of the same compressed size that happened to share them --
 * the first 8 bytes of a zstd frame are a near-constant header -- would have been served stale. */
static uint64_t stream_fingerprint(const void *p, uint32_t n)
{
    const uint8_t *b = (const uint8_t *)p;
    const uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull;
    auto rotl = [](uint64_t x, int r) { return (x << r) | (x >> (64 - r)); };
    auto round1 = [&](uint64_t acc, uint64_t v) { return rotl(acc + v * P2, 31) * P1; };
    uint64_t h;
    uint32_t i = 0;
    if (n >= 32u) {
        uint64_t v1 = P1 + P2, v2 = P2, v3 = 0, v4 = 0 - P1;
        for (; i + 32u <= n; i += 32u) {
            uint64_t w[4];
            memcpy(w, b + i, 32);
            v1 = round1(v1, w[0]); v2 = round1(v2, w[1]); v3 = round1(v3, w[2]); v4 = round1(v4, w[3]);
        }
        h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
        h = (h ^ round1(0, v1)) * P1 + P3;
        h = (h ^ round1(0, v2)) * P1 + P3;
        h = (h ^ round1(0, v3)) * P1 + P3;
        h = (h ^ round1(0, v4)) * P1 + P3;
    } else {
        h = P3;
    }
    h += n;
    for (; i + 8u <= n; i += 8u) { uint64_t w; memcpy(&w, b + i, 8); h = rotl(h ^ round1(0, w), 27) * P1 + P3; }
    for (; i < n; i++) h = rotl(h ^ (b[i] * P3), 11) * P1;
    h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
    return h;
}

static void pool_drop(cryo_codec *c)
{
    if (c->d_pool) { (void)hipStreamSynchronize(c->stream); (void)hipFree(c->d_pool); c->d_pool = nullptr; }
    c->pool_slots.clear();
    c->pool_index.clear();
    c->pool_head = 0;
    c->pool_block = 0;
}

/* (re)shape the pool for this block size; false: no pool (off, or the memory is not there) */
static bool pool_ready(cryo_codec *c, size_t block_size)
{
    if (c->pool_bytes < block_size) { if (c->d_pool) pool_drop(c); return false; }
    const size_t slots = c->pool_bytes / block_size;
    if (c->d_pool && c->pool_block == block_size && c->pool_slots.size() == slots) return true;
    pool_drop(c);
    if (hipMalloc((void **)&c->d_pool, slots * block_size + 64) != hipSuccess) { (void)hipGetLastError(); c->d_pool = nullptr; return false; }
    c->pool_slots.assign(slots, cryo_codec::PoolSlot());
    c->pool_block = block_size;
    return true;
}

static int decompress_blocks_keyed_impl(cryo_codec *c, int method, const uint64_t *keys, const void *const *h_src,
                                        const uint32_t *h_src_size, size_t n, void *const *h_dst, size_t block_size, int32_t *h_status)
{
    DevGuard dev_(c);
    if (!c || !method_ok(method) || !block_size_ok(block_size)) return CRYO_E_ARG;
    if (n == 0) return CRYO_OK;
    if (!keys || !h_src || !h_src_size || !h_dst || !h_status) return CRYO_E_ARG;
    if (!pool_ready(c, block_size)) return decompress_blocks_host(c, method, h_src, h_src_size, n, nullptr, h_dst, block_size, h_status);
    const uint32_t S = (uint32_t)c->pool_slots.size();
    /* who is in the pool already */
    std::vector<uint32_t> slot(n, 0xffffffffu), miss;
    std::vector<uint64_t> fp(n, 0);
    for (size_t i = 0; i < n; i++) {
        if (h_src_size[i] != 0 && !h_src[i]) return CRYO_E_ARG;
        if (!h_dst[i]) return CRYO_E_ARG;
        if (keys[i] != 0 && h_src_size[i] != 0) {
            fp[i] = stream_fingerprint(h_src[i], h_src_size[i]);
            auto it = c->pool_index.find(keys[i]);
            if (it != c->pool_index.end()) {
                const cryo_codec::PoolSlot &ps = c->pool_slots[it->second];
                if (ps.valid && ps.csize == h_src_size[i] && ps.fp == fp[i]) { slot[i] = it->second; h_status[i] = CRYO_OK; continue; }
            }
        }
        miss.push_back((uint32_t)i);
    }
    c->xfer_ctr.pool_hits += n - miss.size();
    c->xfer_ctr.pool_misses += miss.size();
    int rc;
    if ((rc = ensure(c, &c->hb_dst, &c->hb_dst_cap, n * block_size + 64)) != CRYO_OK) return rc;
    if ((rc = ensure_pinned(c, n * block_size + n * 16 + 64)) != CRYO_OK) return rc;
    /* 1. the blocks that are there leave their slots first (a miss below may take a slot over) */
    auto gather = [&](const std::vector<uint32_t> &who) -> int {
        for (size_t a = 0; a < who.size();) {
            /* consecutive blocks of the call, up to 64 per launch, land next to each other in the staging area */
            cryo::GatherSlots gs;
            uint32_t cnt = 0;
            const uint32_t first = who[a];
            while (a < who.size() && cnt < 64u && who[a] == first + cnt) { gs.slot[cnt++] = slot[who[a]]; a++; }
            HIP_TRY(c, cryo::launch_gather_blocks(c->stream, c->d_pool, gs, cnt, c->hb_dst, (uint32_t)block_size, first));
        }
        return CRYO_OK;
    };
    {
        std::vector<uint32_t> hits;
        for (size_t i = 0; i < n; i++) if (slot[i] != 0xffffffffu) hits.push_back((uint32_t)i);
        if ((rc = gather(hits)) != CRYO_OK) return rc;
    }
    /* 2. the others are decoded INTO the pool, at most one pool-full per round, then gathered like the rest */
    std::vector<int32_t> mst(miss.size(), 0);
    for (size_t lo = 0; lo < miss.size(); lo += S) {
        const size_t m = miss.size() - lo < S ? miss.size() - lo : S;
        /* the round's streams: the layout of host_stage.h over this part of the misses */
        const auto size_of = [&](size_t k) { return h_src_size[miss[lo + k]]; };
        const cryo::StreamLayout L(m, size_of);
        if ((rc = ensure(c, &c->hb_src, &c->hb_src_cap, L.bytes() + 64)) != CRYO_OK) return rc;
        if ((rc = ensure(c, &c->hb_meta, &c->hb_meta_cap, m * 16 + 64)) != CRYO_OK) return rc;
        /* staging of the compressed side lives behind the output staging in the pinned buffer */
        if (c->pin_cap < n * block_size + L.bytes() + m * 4 + 128 && (rc = ensure_pinned(c, n * block_size + L.bytes() + m * 4 + 128)) != CRYO_OK) return rc;
        uint8_t *pin = (uint8_t *)c->pin + n * block_size;
        write_staged(c, L, pin, [&](size_t k) { return h_src[miss[lo + k]]; }, size_of, false);
        HIP_TRY(c, hipMemcpyAsync(c->hb_src, pin, L.bytes(), hipMemcpyHostToDevice, c->stream));
        c->xfer_ctr.h2d_bytes += L.bytes();
        int32_t *d_st = (int32_t *)c->hb_meta;
        /* ring slots head .. head+m-1 (two launches when the ring wraps) */
        for (size_t done = 0; done < m;) {
            const uint32_t head = c->pool_head;
            const size_t run = (S - head) < (m - done) ? (S - head) : (m - done);
            for (size_t k = 0; k < run; k++) {
                cryo_codec::PoolSlot &ps = c->pool_slots[head + k];
                if (ps.valid) { auto it = c->pool_index.find(ps.key); if (it != c->pool_index.end() && it->second == head + k) c->pool_index.erase(it); }
                ps.valid = false;
                slot[miss[lo + done + k]] = head + (uint32_t)k;
            }
            rc = cryo_codec_decompress_batch(c, method, c->hb_src, (const uint64_t *)(c->hb_src + L.o_off) + done, (const uint32_t *)(c->hb_src + L.o_sz) + done,
                                             c->d_pool + (size_t)head * block_size, block_size, (uint32_t)block_size, run, d_st + done);
            if (rc != CRYO_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
            c->pool_head = (uint32_t)((head + run) % S);
            done += run;
        }
        HIP_TRY(c, hipMemcpyAsync(pin + L.bytes(), d_st, m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        {
            std::vector<uint32_t> who(miss.begin() + lo, miss.begin() + lo + m);
            if ((rc = gather(who)) != CRYO_OK) return rc;
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream)); /* the statuses of this round, and the compressed staging is free again */
        const int32_t *pst = (const int32_t *)(pin + L.bytes());
        for (size_t k = 0; k < m; k++) {
            const uint32_t i = miss[lo + k];
            h_status[i] = pst[k];
            if (pst[k] == CRYO_OK && keys[i] != 0) {
                cryo_codec::PoolSlot &ps = c->pool_slots[slot[i]];
                ps.key = keys[i]; ps.fp = fp[i]; ps.csize = h_src_size[i]; ps.valid = true;
                c->pool_index[keys[i]] = slot[i];
            }
        }
        c->xfer_ctr.d2h_bytes += m * sizeof(int32_t);
    }
    /* 3. one copy back, then to the destinations */
    HIP_TRY(c, hipMemcpyAsync(c->pin, c->hb_dst, n * block_size, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->xfer_ctr.d2h_bytes += n * block_size;
    return hand_back(c, h_status, h_dst, (const uint8_t *)c->pin, false, n, block_size);
}

extern "C" {
int cryo_codec_decompress_blocks_keyed(cryo_codec *c, int method, const uint64_t *keys, const void *const *h_src,
                                       const uint32_t *h_src_size, size_t n, void *const *h_dst, size_t block_size, int32_t *h_status)
{
    return host_call(c, [&] {
        return decompress_blocks_keyed_impl(c, method, keys, h_src, h_src_size, n, h_dst, block_size, h_status);
    });
}

int cryo_codec_pool_invalidate(cryo_codec *c, uint32_t key_hi, int all_entries)
{
    if (!c) return CRYO_E_ARG;
    return guarded([&] {
        for (size_t k = 0; k < c->pool_slots.size(); k++) {
            cryo_codec::PoolSlot &ps = c->pool_slots[k];
            if (ps.valid && (all_entries || (uint32_t)(ps.key >> 32) == key_hi)) { c->pool_index.erase(ps.key); ps.valid = false; }
        }
        return (int)CRYO_OK;
    });
}

int cryo_codec_get_transfer_counters(const cryo_codec *c, cryo_codec_transfer_counters *out)
{
    if (!c || !out) return CRYO_E_ARG;
    *out = c->xfer_ctr;
    out->pool_blocks = c->pool_index.size();
    out->pool_capacity = c->pool_slots.size();
    return CRYO_OK;
}
} /* extern "C" */

extern "C" {

/* ---- several GPUs behind one call ---- */
struct cryo_multi {
    std::vector<cryo_codec *> h;
    WorkerPool *pool = nullptr; /* one worker per further device */
    char err[320] = {0};
};

int cryo_multi_open(const int *devices, int n_devices, cryo_multi **out)
{
    if (!out || !devices || n_devices <= 0) return CRYO_E_ARG;
    *out = nullptr;
    return guarded([&]() -> int {
        cryo_multi *m = new (std::nothrow) cryo_multi;
        if (!m) return CRYO_E_NOMEM;
        for (int i = 0; i < n_devices; i++) {
            cryo_codec *c = nullptr;
            const int rc = cryo_codec_open(devices[i], &c);
            if (rc != CRYO_OK) { cryo_multi_close(m); return rc; }
            m->h.push_back(c);
        }
        if (n_devices > 1) m->pool = new (std::nothrow) WorkerPool((unsigned)n_devices - 1u); /* none: the shares run one after the other */
        *out = m;
        return CRYO_OK;
    });
}

void cryo_multi_close(cryo_multi *m)
{
    if (!m) return;
    delete m->pool;
    for (cryo_codec *c : m->h) cryo_codec_close(c);
    delete m;
}

int cryo_multi_count(const cryo_multi *m) { return m ? (int)m->h.size() : 0; }
const char *cryo_multi_last_error(const cryo_multi *m) { return m ? m->err : ""; }

} /* extern "C" */
/* The deal, a share's region and the scatter are stated in multi_share.h.  `fn(c, g, idx)` runs the block indices idx of handle g
 * (c), every handle's share on its own host thread; a handle without a share is not touched.  owner(i) names block i's handle.
 * The lowest-numbered failing handle's code is the call's */
template <class Fn, class Owner> static int multi_run(cryo_multi *m, size_t n, const Fn &fn, const Owner &owner)
{
    return guarded([&] {
        const size_t G = m->h.size();
        const std::vector<std::vector<size_t>> share = cryo::deal_shares(n, G, owner);
        std::vector<int> rc(G, CRYO_OK);
        const std::function<void(unsigned)> one = [&](unsigned g) {
            if (!share[g].empty()) {
                rc[g] = guarded([&] { return fn(m->h[g], (size_t)g, share[g]); });
                ws_trim_after_call(m->h[g]); /* the keep limit holds per handle, whoever dispatched the call */
            }
        };
        if (m->pool) m->pool->run((unsigned)G, one);
        else for (unsigned g = 0; g < G; g++) one(g);
        for (size_t g = 0; g < G; g++)
            if (rc[g] != CRYO_OK) {
                snprintf(m->err, sizeof m->err, "device handle %zu: %s", g, cryo_codec_last_error(m->h[g]));
                return rc[g];
            }
        return (int)CRYO_OK;
    });
}
/* round-robin */
template <class Fn> static int multi_run(cryo_multi *m, size_t n, const Fn &fn)
{
    const cryo::RoundRobin deal{n, m->h.size()};
    return multi_run(m, n, fn, [&](size_t i) { return deal.handle_of(i); });
}
namespace {
/* a share's streams: those of the blocks idx[k], in that order */
struct ShareStreams {
    std::vector<const void *> src;
    std::vector<uint32_t> sz;
    ShareStreams(const void *const *h_src, const uint32_t *h_src_size, const std::vector<size_t> &idx)
        : src(cryo::gather(idx, h_src)), sz(cryo::gather(idx, h_src_size)) {}
};
} // namespace
/* how compress, check and the decompress calls begin: CRYO_E_ARG without a handle or with bad arguments, CRYO_OK for no block,
 * CRYO_E_ARG for a null pointer -- in that order -- else MULTI_GO.  The scan calls, recode and fetch keep an order of their own */
enum { MULTI_GO = 1 };
static int multi_begin(const cryo_multi *m, bool args_ok, size_t n, bool ptrs_ok)
{
    if (!m || m->h.empty() || !args_ok) return CRYO_E_ARG;
    if (n == 0) return CRYO_OK;
    return ptrs_ok ? (int)MULTI_GO : (int)CRYO_E_ARG;
}
/* one call on every handle; the first error ends it */
template <class Call> static int multi_each(cryo_multi *m, Call call)
{
    for (cryo_codec *c : m->h) {
        const int rc = call(c);
        if (rc != CRYO_OK) return rc;
    }
    return CRYO_OK;
}
extern "C" {

int cryo_multi_compress_blocks(cryo_multi *m, int method, int param, const void *h_src, size_t block_size, size_t n,
                               void *h_dst, size_t dst_stride, uint32_t *h_out_size)
{
    const int go = multi_begin(m, method_ok(method) && block_size_ok(block_size), n, h_src && h_dst && h_out_size);
    if (go != MULTI_GO) return go;
    if (dst_stride < cryo_codec_bound(method, block_size)) return CRYO_E_DSTSIZE;
    for (cryo_codec *c : m->h) c->vfy_failed = false; /* a handle with no share in this call reports nothing */
    if (m->h.size() == 1) return cryo_codec_compress_blocks(m->h[0], method, param, h_src, block_size, n, h_dst, dst_stride, h_out_size);
    return multi_run(m, n, [&](cryo_codec *c, size_t, const std::vector<size_t> &idx) {
        std::vector<const void *> src(idx.size());
        std::vector<void *> dst(idx.size());
        std::vector<uint32_t> sz(idx.size());
        for (size_t k = 0; k < idx.size(); k++) {
            src[k] = (const uint8_t *)h_src + idx[k] * block_size;
            dst[k] = (uint8_t *)h_dst + idx[k] * dst_stride;
        }
        const int rc = compress_blocks_host(c, method, param, {nullptr, nullptr, 0, src.data(), dst.data()}, block_size, idx.size(), sz.data());
        if (rc == CRYO_OK) cryo::scatter(idx, sz.data(), h_out_size);
        if (rc == CRYO_E_VERIFY && c->vfy_failed) set_verify_failure(c, idx[c->vfy_block], c->vfy_off); /* the index in the whole call */
        return rc;
    });
}

/* one destination per block (h_dst_each) or one strided area (h_dst) */
static int multi_decompress(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                            void *h_dst, void *const *h_dst_each, size_t block_size, int32_t *h_status)
{
    return multi_run(m, n, [&](cryo_codec *c, size_t, const std::vector<size_t> &idx) {
        const ShareStreams in(h_src, h_src_size, idx);
        std::vector<void *> dst(idx.size());
        std::vector<int32_t> st(idx.size());
        for (size_t k = 0; k < idx.size(); k++)
            dst[k] = h_dst_each ? h_dst_each[idx[k]] : (void *)((uint8_t *)h_dst + idx[k] * block_size);
        const int rc = decompress_blocks_host(c, method, in.src.data(), in.sz.data(), idx.size(), nullptr, dst.data(), block_size, st.data());
        if (rc == CRYO_OK) cryo::scatter(idx, st.data(), h_status);
        return rc;
    });
}

int cryo_multi_decompress_blocks(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                                 void *h_dst, size_t block_size, int32_t *h_status)
{
    const int go = multi_begin(m, method_ok(method) && block_size_ok(block_size), n, h_src && h_src_size && h_dst && h_status);
    if (go != MULTI_GO) return go;
    if (m->h.size() == 1) return cryo_codec_decompress_blocks(m->h[0], method, h_src, h_src_size, n, h_dst, block_size, h_status);
    return multi_decompress(m, method, h_src, h_src_size, n, h_dst, nullptr, block_size, h_status);
}

int cryo_multi_decompress_blocks_to(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                                    void *const *h_dst, size_t block_size, int32_t *h_status)
{
    const int go = multi_begin(m, method_ok(method) && block_size_ok(block_size), n, h_src && h_src_size && h_dst && h_status);
    if (go != MULTI_GO) return go;
    if (m->h.size() == 1) return cryo_codec_decompress_blocks_to(m->h[0], method, h_src, h_src_size, n, h_dst, block_size, h_status);
    return multi_decompress(m, method, h_src, h_src_size, n, nullptr, h_dst, block_size, h_status);
}

int cryo_multi_check_blocks(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                            size_t block_size, cryo_check_result *h_result)
{
    const int go = multi_begin(m, method_ok(method) && check_block_size_ok(block_size), n, h_src && h_src_size && h_result);
    if (go != MULTI_GO) return go;
    if (m->h.size() == 1) return cryo_codec_check_blocks(m->h[0], method, h_src, h_src_size, n, block_size, h_result);
    return multi_run(m, n, [&](cryo_codec *c, size_t, const std::vector<size_t> &idx) {
        const ShareStreams in(h_src, h_src_size, idx);
        std::vector<cryo_check_result> res(idx.size());
        const int rc = staged_blocks(c, method, in.src.data(), in.sz.data(), idx.size(), block_size, CheckOp{c, method, block_size, idx.size(), res.data()});
        if (rc == CRYO_OK) cryo::scatter(idx, res.data(), h_result);
        return rc;
    });
}

/* block i -> handle i mod G; handle g packs its share, in block order, into the g-th of G equal 16-byte aligned regions of
 * h_dst (dst_cap / G, rounded down to 16 bytes); the offsets are absolute within h_dst */
int cryo_multi_recode_blocks(cryo_multi *m, int src_method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                             size_t block_size, int dst_method, int dst_param, void *h_dst, size_t dst_cap, uint64_t *h_out_off,
                             uint32_t *h_out_size, int32_t *h_status)
{
    if (!m || m->h.empty()) return CRYO_E_ARG;
    const int ok = recode_args(m->h[0], src_method, dst_method, dst_param, block_size);
    if (ok != CRYO_OK) return ok;
    if (n == 0) return CRYO_OK;
    if (!h_src || !h_src_size || !h_dst || !h_out_off || !h_out_size || !h_status) return CRYO_E_ARG;
    const size_t G = m->h.size();
    if (G == 1)
        return cryo_codec_recode_blocks(m->h[0], src_method, h_src, h_src_size, n, block_size, dst_method, dst_param, h_dst, dst_cap,
                                        h_out_off, h_out_size, h_status);
    const size_t slot = (cryo_codec_bound(dst_method, block_size) + 15) & ~(size_t)15;
    if (dst_cap / G / slot < (n + G - 1) / G) return CRYO_E_DSTSIZE;
    const size_t region = (dst_cap / G) & ~(size_t)15;
    return multi_run(m, n, [&](cryo_codec *c, size_t g, const std::vector<size_t> &idx) {
        const ShareStreams in(h_src, h_src_size, idx);
        std::vector<uint32_t> osz(idx.size());
        std::vector<uint64_t> off(idx.size());
        std::vector<int32_t> st(idx.size());
        const int rc = recode_blocks_impl(c, src_method, in.src.data(), in.sz.data(), idx.size(), block_size, dst_method, dst_param,
                                          (uint8_t *)h_dst + g * region, region, g * region, off.data(), osz.data(), st.data());
        if (rc != CRYO_OK) return rc;
        cryo::scatter(idx, off.data(), h_out_off);
        cryo::scatter(idx, osz.data(), h_out_size);
        cryo::scatter(idx, st.data(), h_status);
        return (int)CRYO_OK;
    });
}

/* block i -> handle i mod G; handle g packs its share, in block order, into a region of block_size * (its blocks) bytes, the
 * regions in handle order; the records come back in call order with offsets that count from h_dst */
int cryo_multi_fetch_blocks(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                            size_t block_size, const uint64_t *h_req_first, const uint16_t *h_pos, void *h_dst, size_t dst_cap,
                            cryo_fetch_result *h_result, uint64_t *h_total)
{
    if (!m || m->h.empty() || !method_ok(method) || !check_block_size_ok(block_size) || !h_total) return CRYO_E_ARG;
    const size_t G = m->h.size();
    if (G == 1)
        return cryo_codec_fetch_blocks(m->h[0], method, h_src, h_src_size, n, block_size, h_req_first, h_pos, h_dst, dst_cap, h_result,
                                       h_total);
    *h_total = 0;
    if (n == 0) return CRYO_OK;
    if (!h_src || !h_src_size || !h_req_first || h_req_first[0] != 0) return CRYO_E_ARG;
    for (size_t i = 0; i < n; i++)
        if (h_req_first[i + 1] < h_req_first[i]) return CRYO_E_ARG;
    if (h_req_first[n] > 0 && (!h_pos || !h_result)) return CRYO_E_ARG;
    if (!h_dst && dst_cap > 0) return CRYO_E_ARG;
    const cryo::RoundRobin deal{n, G};
    std::vector<uint64_t> end(G, 0);
    const int rc = multi_run(m, n, [&](cryo_codec *c, size_t g, const std::vector<size_t> &idx) {
        const cryo::ShareRegion bytes(dst_cap, deal.before(g), idx.size(), block_size);
        const ShareStreams in(h_src, h_src_size, idx);
        /* a block's requests are a range of the call's, of any length: they are gathered and their records scattered range by
         * range here, not by the per-block scatter of multi_share.h */
        std::vector<uint64_t> first(idx.size() + 1, 0);
        for (size_t k = 0; k < idx.size(); k++) first[k + 1] = first[k] + (h_req_first[idx[k] + 1] - h_req_first[idx[k]]);
        std::vector<uint16_t> pos(first.back() ? first.back() : 1);
        std::vector<cryo_fetch_result> res(first.back() ? first.back() : 1);
        for (size_t k = 0; k < idx.size(); k++)
            if (first[k + 1] > first[k])
                memcpy(&pos[first[k]], h_pos + h_req_first[idx[k]], (first[k + 1] - first[k]) * sizeof(uint16_t));
        uint64_t tot = 0;
        const int r = fetch_blocks_impl(c, method, in.src.data(), in.sz.data(), idx.size(), block_size, first.data(), pos.data(),
                                        bytes.in((uint8_t *)h_dst), bytes.cap, bytes.first, res.data(), &tot);
        if (r != CRYO_OK) return r;
        for (size_t k = 0; k < idx.size(); k++)
            if (first[k + 1] > first[k])
                memcpy(h_result + h_req_first[idx[k]], &res[first[k]], (first[k + 1] - first[k]) * sizeof(cryo_fetch_result));
        end[g] = bytes.end(tot);
        return (int)CRYO_OK;
    });
    if (rc != CRYO_OK) return rc;
    *h_total = cryo::last_end(end);
    return CRYO_OK;
}

/* block i -> handle i mod G; handle g packs its share, in block order, into a tuple region of block_size * (its blocks) bytes and
 * a record region of 290 (kHeapMaxItems) * (its blocks) records, whatever the block size, the regions in handle order; the table
 * comes back in call order with `off` and rec_first counting from h_dst and h_rec */
int cryo_multi_filter_blocks(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                             size_t block_size, const cryo_filter *f, void *h_dst, size_t dst_cap, cryo_filter_rec *h_rec,
                             size_t rec_cap, cryo_filter_block *h_blocks, uint64_t *h_total)
{
    uint32_t max_att = 0;
    if (!m || m->h.empty() || filter_blocks_args(method, block_size, f, h_total, &max_att) != CRYO_OK) return CRYO_E_ARG;
    const size_t G = m->h.size();
    if (G == 1)
        return cryo_codec_filter_blocks(m->h[0], method, h_src, h_src_size, n, block_size, f, h_dst, dst_cap, h_rec, rec_cap,
                                        h_blocks, h_total);
    h_total[0] = h_total[1] = 0;
    if (n == 0) return CRYO_OK;
    const bool count_only = (f->flags & CRYO_FILTER_COUNT_ONLY) != 0;
    if (!h_src || !h_src_size || !h_blocks) return CRYO_E_ARG;
    if (!count_only && ((!h_dst && dst_cap > 0) || (!h_rec && rec_cap > 0))) return CRYO_E_ARG;
    const cryo::RoundRobin deal{n, G};
    std::vector<uint64_t> end_b(G, 0), end_r(G, 0);
    const int rc = multi_run(m, n, [&](cryo_codec *c, size_t g, const std::vector<size_t> &idx) {
        const cryo::ShareRegion bytes(dst_cap, deal.before(g), idx.size(), block_size);
        const cryo::ShareRegion recs(rec_cap, deal.before(g), idx.size(), cryo::kHeapMaxItems);
        const ShareStreams in(h_src, h_src_size, idx);
        std::vector<cryo_filter_block> rows(idx.size());
        uint64_t tot[2] = {0, 0};
        const int r = filter_blocks_impl(c, method, in.src.data(), in.sz.data(), idx.size(), block_size, f, bytes.in((uint8_t *)h_dst),
                                         bytes.cap, bytes.first, recs.in(h_rec), recs.cap, recs.first, rows.data(), tot);
        if (r != CRYO_OK) return r;
        cryo::scatter(idx, rows.data(), h_blocks);
        end_b[g] = bytes.end(tot[0]);
        end_r[g] = recs.end(tot[1]);
        return (int)CRYO_OK;
    });
    if (rc != CRYO_OK) return rc;
    h_total[0] = cryo::last_end(end_b);
    h_total[1] = cryo::last_end(end_r);
    return CRYO_OK;
}

/* block i -> handle i mod G; rows and cells are fixed-size per block and land in call order */
int cryo_multi_agg_blocks(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                          size_t block_size, const cryo_filter *f, const cryo_agg *agg, cryo_agg_block *h_blocks,
                          cryo_agg_cell *h_cells)
{
    uint32_t max_att = 0;
    if (!m || m->h.empty() || agg_blocks_args(method, block_size, f, agg, &max_att) != CRYO_OK) return CRYO_E_ARG;
    const size_t G = m->h.size();
    if (G == 1) return cryo_codec_agg_blocks(m->h[0], method, h_src, h_src_size, n, block_size, f, agg, h_blocks, h_cells);
    if (n == 0) return CRYO_OK;
    if (!h_src || !h_src_size || !h_blocks || !h_cells) return CRYO_E_ARG;
    const size_t nc = agg->ncols;
    return multi_run(m, n, [&](cryo_codec *c, size_t, const std::vector<size_t> &idx) {
        const ShareStreams in(h_src, h_src_size, idx);
        std::vector<cryo_agg_block> rows(idx.size());
        std::vector<cryo_agg_cell> cells(idx.size() * nc);
        const int r = agg_blocks_impl(c, method, in.src.data(), in.sz.data(), idx.size(), block_size, f, agg, rows.data(), cells.data());
        if (r != CRYO_OK) return r;
        cryo::scatter(idx, rows.data(), h_blocks);
        cryo::scatter(idx, cells.data(), h_cells, nc);
        return (int)CRYO_OK;
    });
}

/* block i -> handle i mod G; every handle groups its share into buffers of its own, then the host lays records and cells back
 * into call order and rebases first_group: the single-handle call's output, byte for byte */
int cryo_multi_group_blocks(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                            size_t block_size, const cryo_filter *f, const cryo_group *grp, const cryo_agg *agg,
                            cryo_group_block *h_blocks, cryo_group_rec *h_groups, size_t group_cap, cryo_agg_cell *h_cells,
                            uint64_t *h_total)
{
    uint32_t max_att = 0, nc = 0, text = 0;
    if (!m || m->h.empty() || group_blocks_args(method, block_size, f, grp, agg, h_total, &max_att, &nc, &text) != CRYO_OK) return CRYO_E_ARG;
    nc += (uint32_t)__builtin_popcount(text); /* from here on a group's cells: the key cells travel with the aggregate cells */
    const size_t G = m->h.size();
    if (G == 1)
        return cryo_codec_group_blocks(m->h[0], method, h_src, h_src_size, n, block_size, f, grp, agg, h_blocks, h_groups, group_cap,
                                       h_cells, h_total);
    *h_total = 0;
    if (n == 0) return CRYO_OK;
    if (!h_src || !h_src_size || !h_blocks || (group_cap > 0 && (!h_groups || (nc > 0 && !h_cells)))) return CRYO_E_ARG;
    const size_t S = cryo::filter_side_stride((uint32_t)block_size);
    std::vector<std::vector<cryo_group_block>> rows(G);
    std::vector<std::vector<cryo_group_rec>> recs(G);
    std::vector<std::vector<cryo_agg_cell>> cells(G);
    std::vector<uint64_t> tot(G, 0);
    const int rc = multi_run(m, n, [&](cryo_codec *c, size_t g, const std::vector<size_t> &idx) {
        const ShareStreams in(h_src, h_src_size, idx);
        /* a share's room: its worst case, or the whole call's room when that is less -- a share that needs more than the
         * call has room for fails the call as the single handle would */
        const size_t cap = idx.size() * S < group_cap ? idx.size() * S : group_cap;
        rows[g].resize(idx.size());
        recs[g].resize(cap ? cap : 1);
        cells[g].resize(cap * nc ? cap * nc : 1);
        return group_blocks_impl(c, method, in.src.data(), in.sz.data(), idx.size(), block_size, f, grp, agg, rows[g].data(),
                                 recs[g].data(), cap, cells[g].data(), &tot[g]);
    });
    uint64_t total = 0;
    for (size_t g = 0; g < G; g++) total += tot[g];
    if (rc != CRYO_OK) return rc;
    *h_total = total;
    if (total > group_cap) return CRYO_E_DSTSIZE;
    const cryo::RoundRobin deal{n, G};
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        const size_t g = deal.handle_of(i), k = deal.entry_of(i);
        cryo_group_block row = rows[g][k];
        if (row.n_groups) {
            memcpy(h_groups + at, &recs[g][row.first_group], row.n_groups * sizeof(cryo_group_rec));
            if (nc) memcpy(h_cells + at * nc, &cells[g][row.first_group * nc], row.n_groups * nc * sizeof(cryo_agg_cell));
        }
        row.first_group = at;
        at += row.n_groups;
        h_blocks[i] = row;
    }
    return CRYO_OK;
}

/* block i -> handle i mod G; handle g projects its share, in block order, into a row region and a record region of 290
 * (kHeapMaxItems) * (its blocks) entries each, whatever the block size, the regions in handle order; the table comes back in call
 * order with row_first and rec_first counting from h_rows and h_rec */
int cryo_multi_project_blocks(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n,
                              size_t block_size, const cryo_filter *f, const cryo_project *prj, void *h_rows, size_t row_cap,
                              cryo_project_rec *h_rec, size_t rec_cap, cryo_project_block *h_blocks, uint64_t *h_total)
{
    uint32_t max_att = 0;
    ProjectTab pt;
    if (!m || m->h.empty() || project_blocks_args(method, block_size, f, prj, h_total, &max_att, &pt) != CRYO_OK) return CRYO_E_ARG;
    const size_t G = m->h.size();
    if (G == 1)
        return cryo_codec_project_blocks(m->h[0], method, h_src, h_src_size, n, block_size, f, prj, h_rows, row_cap, h_rec, rec_cap,
                                         h_blocks, h_total);
    h_total[0] = h_total[1] = 0;
    if (n == 0) return CRYO_OK;
    if (!h_src || !h_src_size || !h_blocks || (!h_rows && row_cap > 0) || (!h_rec && rec_cap > 0)) return CRYO_E_ARG;
    const cryo::RoundRobin deal{n, G};
    std::vector<uint64_t> end_w(G, 0), end_r(G, 0);
    const int rc = multi_run(m, n, [&](cryo_codec *c, size_t g, const std::vector<size_t> &idx) {
        const cryo::ShareRegion rows(row_cap, deal.before(g), idx.size(), cryo::kHeapMaxItems);
        const cryo::ShareRegion recs(rec_cap, deal.before(g), idx.size(), cryo::kHeapMaxItems);
        const ShareStreams in(h_src, h_src_size, idx);
        std::vector<cryo_project_block> table(idx.size());
        uint64_t tot[2] = {0, 0};
        const int r = project_blocks_impl(c, method, in.src.data(), in.sz.data(), idx.size(), block_size, f, prj,
                                          rows.in((uint8_t *)h_rows, pt.row_bytes), rows.cap, rows.first, recs.in(h_rec), recs.cap,
                                          recs.first, table.data(), tot);
        if (r != CRYO_OK) return r;
        cryo::scatter(idx, table.data(), h_blocks);
        end_w[g] = rows.end(tot[0]);
        end_r[g] = recs.end(tot[1]);
        return (int)CRYO_OK;
    });
    if (rc != CRYO_OK) return rc;
    h_total[0] = cryo::last_end(end_w);
    h_total[1] = cryo::last_end(end_r);
    return CRYO_OK;
}

/* block i -> handle i mod G; handle g ranks its share, in block order, into one region of min(limit, 290) * (its blocks) entries of
 * rows and records alike, the regions in handle order; the table comes back in call order with row_first counting from h_rows */
int cryo_multi_topn_blocks(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size, size_t n, size_t block_size,
                           const cryo_filter *f, const cryo_order *ord, const cryo_project *prj, void *h_rows, cryo_topn_rec *h_rec,
                           size_t row_cap, cryo_topn_block *h_blocks, uint64_t *h_total)
{
    uint32_t max_att = 0;
    TopnTab tt;
    if (!m || m->h.empty() || topn_blocks_args(method, block_size, f, ord, prj, h_total, &max_att, &tt) != CRYO_OK) return CRYO_E_ARG;
    const size_t G = m->h.size();
    if (G == 1) return cryo_codec_topn_blocks(m->h[0], method, h_src, h_src_size, n, block_size, f, ord, prj, h_rows, h_rec, row_cap, h_blocks, h_total);
    *h_total = 0;
    if (n == 0) return CRYO_OK;
    if (!h_src || !h_src_size || !h_blocks || ((!h_rows || !h_rec) && row_cap > 0)) return CRYO_E_ARG;
    const cryo::RoundRobin deal{n, G};
    const uint64_t per_block = topn_per_block(tt.limit, cryo::kHeapMaxItems);
    std::vector<uint64_t> end_w(G, 0);
    const int rc = multi_run(m, n, [&](cryo_codec *c, size_t g, const std::vector<size_t> &idx) {
        const cryo::ShareRegion rows(row_cap, deal.before(g), idx.size(), per_block);
        const ShareStreams in(h_src, h_src_size, idx);
        std::vector<cryo_topn_block> table(idx.size());
        uint64_t tot = 0;
        const int r = topn_blocks_impl(c, method, in.src.data(), in.sz.data(), idx.size(), block_size, f, ord, prj,
                                       rows.in((uint8_t *)h_rows, tt.row_bytes), rows.in(h_rec), rows.cap, rows.first, table.data(), &tot);
        if (r != CRYO_OK) return r;
        cryo::scatter(idx, table.data(), h_blocks);
        end_w[g] = rows.end(tot);
        return (int)CRYO_OK;
    });
    if (rc != CRYO_OK) return rc;
    *h_total = cryo::last_end(end_w);
    return CRYO_OK;
}

int cryo_multi_decompress_blocks_keyed(cryo_multi *m, int method, const uint64_t *keys, const void *const *h_src,
                                       const uint32_t *h_src_size, size_t n, void *const *h_dst, size_t block_size, int32_t *h_status)
{
    const int go = multi_begin(m, method_ok(method) && block_size_ok(block_size), n, keys && h_src && h_src_size && h_dst && h_status);
    if (go != MULTI_GO) return go;
    if (m->h.size() == 1) return cryo_codec_decompress_blocks_keyed(m->h[0], method, keys, h_src, h_src_size, n, h_dst, block_size, h_status);
    const size_t G = m->h.size();
    return multi_run(
        m, n,
        [&](cryo_codec *c, size_t, const std::vector<size_t> &idx) {
            const ShareStreams in(h_src, h_src_size, idx);
            const std::vector<void *> dst = cryo::gather(idx, h_dst);
            const std::vector<uint64_t> ky = cryo::gather(idx, keys);
            std::vector<int32_t> st(idx.size());
            const int r = decompress_blocks_keyed_impl(c, method, ky.data(), in.src.data(), in.sz.data(), idx.size(), dst.data(),
                                                       block_size, st.data());
            if (r == CRYO_OK) cryo::scatter(idx, st.data(), h_status);
            return r;
        },
        [&](size_t i) { return cryo::keyed_owner(keys[i], i, G); });
}

int cryo_multi_set_option(cryo_multi *m, int option, int64_t value)
{
    if (!m || m->h.empty()) return CRYO_E_ARG;
    /* a pool capacity is the total over the handles */
    const int64_t v = option == CRYO_OPT_POOL_BYTES ? value / (int64_t)m->h.size() : value;
    return multi_each(m, [&](cryo_codec *c) { return cryo_codec_set_option(c, option, v); });
}

int cryo_multi_trim(cryo_multi *m)
{
    return m ? multi_each(m, [](cryo_codec *c) { return cryo_codec_trim(c); }) : (int)CRYO_E_ARG;
}

int cryo_multi_pool_invalidate(cryo_multi *m, uint32_t key_hi, int all_entries)
{
    return m ? multi_each(m, [&](cryo_codec *c) { return cryo_codec_pool_invalidate(c, key_hi, all_entries); }) : (int)CRYO_E_ARG;
}

int cryo_multi_last_verify_failure(const cryo_multi *m, uint64_t *block, uint32_t *first_mismatch)
{
    if (!m) return CRYO_E_ARG;
    const cryo_codec *hit = nullptr;
    for (const cryo_codec *c : m->h)
        if (c->vfy_failed && (!hit || c->vfy_block < hit->vfy_block)) hit = c;
    return hit ? cryo_codec_last_verify_failure(hit, block, first_mismatch) : 0;
}

int cryo_multi_get_transfer_counters(const cryo_multi *m, cryo_codec_transfer_counters *out)
{
    if (!m || !out) return CRYO_E_ARG;
    memset(out, 0, sizeof *out);
    for (const cryo_codec *c : m->h) {
        cryo_codec_transfer_counters t;
        if (cryo_codec_get_transfer_counters(c, &t) != CRYO_OK) return CRYO_E_ARG;
        out->h2d_bytes += t.h2d_bytes; out->d2h_bytes += t.d2h_bytes; out->pool_hits += t.pool_hits; out->pool_misses += t.pool_misses;
        out->pool_blocks += t.pool_blocks; out->pool_capacity += t.pool_capacity;
    }
    return CRYO_OK;
}

/* ---- helpers ---- */
int cryo_codec_synth_batch(cryo_codec *c, uint64_t seed, uint64_t first_block, uint64_t block_step,
                           uint64_t n_blocks, uint32_t block_size, int dist, void *d_dst, uint64_t dst_stride)
{
    DevGuard dev_(c);
    if (!c || block_size < 64 || block_size > kMaxBlockSize || dist < 0 || dist > 4) return CRYO_E_ARG;
    if (n_blocks == 0) return CRYO_OK;
    if (!d_dst || dst_stride < block_size) return CRYO_E_ARG;
    HIP_TRY(c, cryo::launch_synth(c->stream, seed, first_block, block_step ? block_step : 1, n_blocks, block_size, dist,
                                  (uint8_t *)d_dst, dst_stride));
    c->ctr.launches++;
    return CRYO_OK;
}

uint32_t cryo_codec_lz4_index_cap(uint32_t block_size)
{
    if (block_size == 0 || block_size > kMaxBlockSize) return 0;
    return cryo::lz4_index_layout(1, block_size, 1).cap;
}

int cryo_codec_lz4_index_rows(cryo_codec *c, const void *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                              uint32_t block_size, uint64_t n_blocks, int form, uint16_t *d_entries, uint32_t *d_counts)
{
    DevGuard dev_(c);
    if (!c || block_size == 0 || block_size > kMaxBlockSize || form < 0 || form > 2) return CRYO_E_ARG;
    if (n_blocks == 0) return CRYO_OK;
    if (!d_src || !d_src_off || !d_src_size || !d_entries || !d_counts) return CRYO_E_ARG;
    const cryo::Lz4IndexLayout L = cryo::lz4_index_layout(n_blocks, block_size, 1);
    int rc = ensure_ws(c, L.bytes);
    if (rc != CRYO_OK) return rc;
    HIP_TRY(c, cryo::launch_lz4_index_form(c->stream, (const uint8_t *)d_src, d_src_off, d_src_size, n_blocks, block_size, c->d_ws, L, form,
                                           c->lz4_opts.cus));
    HIP_TRY(c, hipMemcpyAsync(d_entries, c->d_ws, (size_t)n_blocks * L.cap * sizeof(uint16_t), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, cryo::launch_lz4_index_counts(c->stream, c->d_ws, L, n_blocks, d_counts));
    c->ctr.launches++;
    return CRYO_OK;
}

int cryo_codec_checksum_batch(cryo_codec *c, const void *d_src, uint64_t src_stride,
                              const uint32_t *d_sizes, uint32_t fixed_size, uint64_t n_blocks,
                              uint64_t *d_sums)
{
    DevGuard dev_(c);
    if (!c) return CRYO_E_ARG;
    if (n_blocks == 0) return CRYO_OK;
    if (!d_src || !d_sums) return CRYO_E_ARG;
    HIP_TRY(c, cryo::launch_checksum(c->stream, (const uint8_t *)d_src, src_stride, d_sizes, fixed_size,
                                     n_blocks, d_sums));
    c->ctr.launches++;
    return CRYO_OK;
}

int cryo_codec_compare_batch(cryo_codec *c, const void *d_a, uint64_t a_stride, const void *d_b,
                             uint64_t b_stride, uint32_t block_size, uint64_t n_blocks,
                             uint64_t *d_mismatch)
{
    DevGuard dev_(c);
    if (!c || block_size > kMaxBlockSize) return CRYO_E_ARG;
    if (n_blocks == 0) return CRYO_OK;
    if (!d_a || !d_b || !d_mismatch) return CRYO_E_ARG;
    HIP_TRY(c, cryo::launch_compare(c->stream, (const uint8_t *)d_a, a_stride, (const uint8_t *)d_b,
                                    b_stride, block_size, n_blocks, d_mismatch));
    c->ctr.launches++;
    return CRYO_OK;
}

static int sync_all_streams(cryo_codec *c)
{
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->xfer) HIP_TRY(c, hipStreamSynchronize(c->xfer));
    for (int l = 0; l < cryo::kZstdLanes; l++) {
        if (c->aux.lane[l]) HIP_TRY(c, hipStreamSynchronize(c->aux.lane[l]));
        if (c->aux.side[l]) HIP_TRY(c, hipStreamSynchronize(c->aux.side[l]));
    }
    if (c->lz4_opts.side) HIP_TRY(c, hipStreamSynchronize(c->lz4_opts.side));
    return CRYO_OK;
}

int cryo_codec_debug_fill(cryo_codec *c, int value, cryo_codec_fill_report *out)
{
    DevGuard dev_(c);
    if (!c || value < 0 || value > 255) return CRYO_E_ARG;
    int rc = sync_all_streams(c);
    if (rc != CRYO_OK) return rc;
    cryo_codec_fill_report r = {};
    struct { void *p; size_t cap; uint64_t *filled; } dev[] = {
        {c->d_ws, c->ws_cap, &r.d_ws},         {c->d_vfy, c->vfy_cap, &r.d_vfy},       {c->d_rec, c->rec_cap, &r.d_rec},
        {c->hb_src, c->hb_src_cap, &r.hb_src}, {c->hb_dst, c->hb_dst_cap, &r.hb_dst},  {c->hb_meta, c->hb_meta_cap, &r.hb_meta},
        {c->d_in, c->in_cap, &r.d_in},         {c->d_out, c->out_cap, &r.d_out},       {c->d_off, sizeof(uint64_t), &r.d_scalars},
        {c->d_size, sizeof(uint32_t), &r.d_scalars}, {c->d_status, sizeof(int32_t), &r.d_scalars},
        {c->d_keytab, kDescTablesBytes, &r.d_keytab},
    };
    for (auto &b : dev) {
        if (!b.p || b.cap == 0) continue;
        HIP_TRY(c, hipMemsetAsync(b.p, value, b.cap, c->stream));
        *b.filled += b.cap;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->pin && c->pin_cap) { memset(c->pin, value, c->pin_cap); r.pin = c->pin_cap; }
    for (int i = 0; i < 4; i++)
        if (c->pipe_pin[i] && c->pipe_pin_cap[i]) { memset(c->pipe_pin[i], value, c->pipe_pin_cap[i]); r.pipe_pin[i] = c->pipe_pin_cap[i]; }
    if (out) *out = r;
    return CRYO_OK;
}

/* ---- timing ---- */
int cryo_codec_timer_start(cryo_codec *c)
{
    DevGuard dev_(c);
    if (!c) return CRYO_E_ARG;
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    return CRYO_OK;
}
int cryo_codec_timer_stop(cryo_codec *c, float *ms)
{
    DevGuard dev_(c);
    if (!c || !ms) return CRYO_E_ARG;
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    HIP_TRY(c, hipEventSynchronize(c->ev1));
    HIP_TRY(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return CRYO_OK;
}

int cryo_codec_get_counters(const cryo_codec *c, cryo_codec_counters *out)
{
    if (!c || !out) return CRYO_E_ARG;
    *out = c->ctr;
    return CRYO_OK;
}

} /* extern "C" */
