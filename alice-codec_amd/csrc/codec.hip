// Host side of libalice_codec.so: device/stream/memory plumbing, the chunk object and
// `.alc` (de)serialiser, the FrameEncoder / FrameDecoder orchestration and the C ABI
// declared in include/alice_codec.h.
//
// Reference behaviour restated (reference checkout, file:line):
//   FrameEncoder::encode   src/pipeline.rs:377-507     FrameDecoder::decode  src/pipeline.rs:537-624
//   EncodedChunk::to_bytes src/pipeline.rs:200-226     from_bytes            src/pipeline.rs:235-313
//   C ABI                  src/ffi.rs:12-315
//
// Every compute step is a HIP kernel; nothing here falls back to the CPU.  If no HIP
// device is usable the entry points fail (NULL / error code) -- loudly via
// alice_codec_last_error().
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <iterator>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/alice_codec.h"
#include "../../include/alice_codec_test.h"
#include "common.h"
#include "kernels.h"

using namespace alice;

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------

namespace {

thread_local int tl_err = kOk;
thread_local std::string tl_msg;

int fail(int code, const std::string& msg) {
    tl_err = code;
    tl_msg = msg;
    return code;
}
void clear_error() { tl_err = kOk; tl_msg.clear(); }

// ALICE_CODEC_DEBUG set: the hub's launches and every chain's result go to stderr.  Read once: the library calls setenv
// (widen_hw_queues_once), and getenv concurrent with setenv is not thread-safe.
bool debug_on() {
    static const bool on = getenv("ALICE_CODEC_DEBUG") != nullptr;
    return on;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess) {                                                               \
            int code__ = (e__ == hipErrorOutOfMemory) ? (int)kOutOfMemory : (int)kDeviceError; \
            return fail(code__, std::string(#expr) + ": " + hipGetErrorString(e__));         \
        }                                                                                      \
    } while (0)

// ------------------------------------------------------------------------------------------
// device, stream, memory pool
// ------------------------------------------------------------------------------------------

thread_local int tl_device = -1;         // -1: not chosen yet (device 0 on first use)
// stream the work of the current entry point runs on: buffers allocated meanwhile remember it and drain it before they
// go back to the pool (an error return may leave kernels in flight on them)
thread_local hipStream_t tl_scope_stream = nullptr;

// HIP maps streams onto hardware queues, 4 by default, and kernels of streams that share a queue run one after the other.
// A chain kernel runs for seconds, so with the default only four host threads' calls make progress at a time (measured:
// 64 threads through alice_codec_encode64 ran 4 chunks at a time).  Ask for more before the runtime creates its queues --
// 8 is what the device honours (32 behaved like 8); a host that has initialised HIP already, or set the variable itself,
// keeps what it has.  ALICE_CODEC_KEEP_HW_QUEUES=1 leaves the environment alone.
void widen_hw_queues_once() {
    static const bool done = [] {
        if (!getenv("ALICE_CODEC_KEEP_HW_QUEUES")) setenv("GPU_MAX_HW_QUEUES", "8", 0);
        return true;
    }();
    (void)done;
}

int ensure_device() {
    widen_hw_queues_once();
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(kDeviceError, "no usable HIP device: this library has no CPU fallback (" +
                                      std::string(e != hipSuccess ? hipGetErrorString(e) : "device count 0") + ")");
    if (tl_device < 0) {
        int cur = 0;
        if (hipGetDevice(&cur) == hipSuccess) tl_device = cur; else tl_device = 0;
    }
    if (tl_device >= count) return fail(kDeviceError, "device index out of range");
    HIP_TRY(hipSetDevice(tl_device));
    return kOk;
}

// the stream this thread's host-side work goes to: one of the chain hub's shared short streams (defined below ChainHub)
int get_stream(hipStream_t* out);

// Size-bucketed cache of device allocations.  hipFree waits for EVERY kernel running on the device -- with other threads'
// chains in flight that is seconds (64 host threads through alice_codec_encode64 took 49 s instead of 6 while the cache
// was capped at 8 GB and every call's buffers were freed behind it) -- so blocks are kept up to half of the device's
// memory and given back only by alice_codec_trim() or when an allocation fails.
class DevicePool {
public:
    int alloc(size_t bytes, void** out) {
        const size_t b = bucket(bytes);
        int dev = tl_device;
        {
            std::lock_guard<std::mutex> g(mu_);
            auto it = free_.find({dev, b});
            if (it != free_.end() && !it->second.empty()) {
                *out = it->second.back();
                it->second.pop_back();
                cached_ -= b;
                return kOk;
            }
        }
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, b);
        if (e != hipSuccess) {
            trim();
            e = hipMalloc(&p, b);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(kOutOfMemory, "hipMalloc of " + std::to_string(b) + " bytes failed: " + hipGetErrorString(e));
        }
        *out = p;
        return kOk;
    }
    // dev = the device the block was allocated on (the releasing thread may have moved on to another one)
    void release(void* p, size_t bytes, int dev) {
        if (!p) return;
        const size_t b = bucket(bytes);
        std::lock_guard<std::mutex> g(mu_);
        // (very large blocks -- a batch's symbol volume -- only ever fit the batch that made them: not worth keeping)
        if (b > (size_t(8) << 30) || cached_ + b > max_cached()) { (void)hipFree(p); return; }
        free_[{dev, b}].push_back(p);
        cached_ += b;
    }
    void trim() {
        std::lock_guard<std::mutex> g(mu_);
        for (auto& kv : free_) for (void* p : kv.second) (void)hipFree(p);
        free_.clear();
        cached_ = 0;
    }
    size_t cached() { std::lock_guard<std::mutex> g(mu_); return cached_; }
private:
    static size_t bucket(size_t bytes) {
        if (bytes < 256) bytes = 256;
        if (bytes <= (1u << 20)) {  // next power of two
            size_t b = 256;
            while (b < bytes) b <<= 1;
            return b;
        }
        const size_t g = size_t(2) << 20;  // 2 MiB granules
        return (bytes + g - 1) / g * g;
    }
    // half of the device's memory (of the first device asked about: the devices of a node are alike), at least 8 GB
    static size_t max_cached() {
        static const size_t cap = [] {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return size_t(8) << 30; }
            return std::max(total_b / 2, size_t(8) << 30);
        }();
        return cap;
    }
    std::mutex mu_;
    std::map<std::pair<int, size_t>, std::vector<void*>> free_;
    size_t cached_ = 0;
};

DevicePool& pool() {
    static DevicePool* p = new DevicePool();  // leaked on purpose: no HIP calls during static destruction
    return *p;
}

struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
    int dev = 0;                // device the block lives on
    hipStream_t st = nullptr;   // stream whose work may still touch it
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }
    int alloc(size_t bytes) {
        reset();
        if (bytes == 0) bytes = 16;
        int rc = pool().alloc(bytes, &p);
        if (rc == kOk) { n = bytes; dev = tl_device; st = tl_scope_stream; }
        return rc;
    }
    // The pool is shared by all threads, each with a stream of its own: a block must be idle before another thread can
    // get it.  On the normal paths the stream has been synchronised already and this returns at once.
    void reset() {
        if (p) {
            if (st) (void)hipStreamSynchronize(st);
            pool().release(p, n, dev);
        }
        p = nullptr; n = 0; st = nullptr;
    }
    template <typename T> T* as() const { return (T*)p; }
};

}  // namespace
// RansDecoder (src/rans.rs:321-326: state, input, pos).  The input is uploaded once, at the first decode, and stays on the
// device the object was first used on until the object is destroyed (decode() one symbol at a time must not re-send it).
struct AliceRansDecoder {
    std::vector<uint8_t> input;
    uint32_t state = 0;
    uint64_t pos = 0;
    bool started = false;
    DevBuf d_input;
    int device = -1;
};
namespace {

// Entry points that run on a CALLER's stream name it here for the duration of the call: buffers allocated meanwhile
// remember it (DevBuf::alloc) and drain it before they go back to the pool.  Cleared on return, so that a later call of
// the same thread never tags its buffers with a stream the caller may have destroyed since.
struct ScopeStream {
    explicit ScopeStream(hipStream_t s) { tl_scope_stream = s; }
    ~ScopeStream() { tl_scope_stream = nullptr; }
    ScopeStream(const ScopeStream&) = delete;
    ScopeStream& operator=(const ScopeStream&) = delete;
};

// Entry points that work on an object tied to a device (a batch) switch this thread to it for the call.
struct DeviceScope {
    int saved;
    bool ok;
    explicit DeviceScope(int device) : saved(tl_device), ok(true) {
        tl_device = device;
        if (ensure_device() != kOk) ok = false;
    }
    ~DeviceScope() {
        tl_device = saved;
        if (saved >= 0) (void)hipSetDevice(saved);
    }
};

#define TRY(expr) do { int rc__ = (expr); if (rc__ != kOk) return rc__; } while (0)

// ------------------------------------------------------------------------------------------
// ChainHub: the chain launches of concurrent host calls, merged
//
// A chain kernel runs for seconds and kernels of streams that share a hardware queue run one after the other; the device
// grants eight queues.  With a stream per calling thread, 64 threads in alice_codec_encode64 therefore had eight chunks'
// chains running at a time (398 Mpix/s; profiles/r03_host_api_1080p64_8_hw_queues.json) on a GPU that holds 341 chunks'
// chains.  The whole-chunk host entry points (encode / decode of one chunk, of many chunks) now run like this:
//   * everything short -- copies, transforms, table builds, stream compaction -- goes to one of kShort streams shared by
//     all calling threads; nothing on them ever waits for a chain, so they stay short;
//   * a call hands its chains (descriptors + an event that says their inputs are complete) to the hub and sleeps; one of
//     the waiting threads, the leader, merges everything that is pending into ONE launch on one of kLanes lane streams and
//     every member then waits on the host for that launch's event before it queues its own tail on its short stream;
//   * kShort + kLanes = 7 streams in all, so every one of them owns a hardware queue as long as the host process does not
//     crowd the eight with streams of its own.
// Gathering: a call announces itself when it enters (HubTicket) and the leader waits for the announced calls to arrive, but
// never longer than a tenth of its own chains' run time (a call with a small chunk never waits for a large one's upload);
// a lone caller launches at once.  When all lanes are busy the pending calls pile up and leave together with the next
// free lane.  (Round 3 first tried a combiner that kept the callers' own streams: their short work then sat in hardware
// queues behind other callers' merged chains, and it was slower than no combiner at all:
// profiles/r03_host_api_1080p64_chain_combiner_rejected.json.)
// ------------------------------------------------------------------------------------------
constexpr int kHubShort = 3, kHubLanes = 4, kHubMaxMerged = 1023;   // <= 1023 chains: the one-chain-per-SIMD instances

struct HubLaunch {
    hipEvent_t done = nullptr;
    DevBuf descs;
    std::vector<RansEncodeDesc> enc;      // host copies: alive until the launch is over
    std::vector<RansDecodeDesc> dec;
    int rc = kOk;
    std::string msg;
    ~HubLaunch() { if (done) (void)hipEventDestroy(done); }
};

struct HubJob {
    bool encode = true;
    std::vector<RansEncodeDesc> enc;
    std::vector<RansDecodeDesc> dec;
    hipEvent_t ready = nullptr;           // recorded by the caller on its short stream: the chains' inputs are complete
    double seconds = 0.0;                 // rough run time of the chains (bounds the gather wait)
    std::shared_ptr<HubLaunch> launch;    // set by the leader
    size_t chains() const { return encode ? enc.size() : dec.size(); }
};

class ChainHub {
public:
    static ChainHub* of_device(int device) {
        static std::mutex mu;
        static std::map<int, ChainHub*> hubs;   // leaked on purpose: no HIP calls during static destruction
        std::lock_guard<std::mutex> g(mu);
        auto it = hubs.find(device);
        if (it != hubs.end()) return it->second;
        ChainHub* h = new ChainHub();
        for (auto& s : h->short_) if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) h->ok_ = false;
        for (auto& l : h->lanes_) if (hipStreamCreateWithFlags(&l.st, hipStreamNonBlocking) != hipSuccess) h->ok_ = false;
        hubs[device] = h;
        return h;
    }
    bool ok() const { return ok_; }
    hipStream_t short_stream() {
        static std::atomic<unsigned> next{0};
        thread_local unsigned mine = next.fetch_add(1u);
        return short_[mine % kHubShort];
    }
    // Admission: the whole-chunk calls in flight together must fit the device.  A call states what it is about to allocate
    // and waits here while the calls already inside hold too much (a call alone always enters); without this a thread pool
    // larger than the memory allows would turn the surplus calls into out-of-memory errors instead of a queue.
    void admit(size_t bytes) {
        std::unique_lock<std::mutex> lk(adm_mu_);
        const uint64_t my_turn = next_turn_++;   // first come, first admitted: a large call is not starved by a stream of small ones
        adm_cv_.wait(lk, [&] {
            if (my_turn != serving_) return false;
            if (in_flight_ == 0) {
                // nobody inside: what the device has free now plus what the pool would hand back is the budget (90 % of it)
                if (!budget_fixed_) {
                    size_t free_b = 0, total_b = 0;
                    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = size_t(16) << 30; }
                    budget_ = (free_b + pool().cached()) / 10 * 9;
                }
                return true;
            }
            return in_flight_ + bytes <= budget_;
        });
        in_flight_ += bytes;
        ++serving_;
        adm_cv_.notify_all();
        if (debug_on())
            fprintf(stderr, "[alice] hub: admitted %.2f GB, %.2f GB in flight of a budget of %.2f GB\n", bytes / 1e9, in_flight_ / 1e9, budget_ / 1e9);
    }
    void leave(size_t bytes) { { std::lock_guard<std::mutex> g(adm_mu_); in_flight_ -= std::min(in_flight_, bytes); } adm_cv_.notify_all(); }
    void set_budget(size_t bytes) { { std::lock_guard<std::mutex> g(adm_mu_); budget_ = bytes; budget_fixed_ = bytes != 0; } adm_cv_.notify_all(); }
    void announce() { std::lock_guard<std::mutex> g(mu_); ++expected_; }
    void arrived_or_gone() { { std::lock_guard<std::mutex> g(mu_); if (expected_ > 0) --expected_; } cv_.notify_all(); }

    // Hands the job's chains to the next merged launch and returns when they have run.  The caller has recorded job.ready.
    int run(HubJob& job) {
        std::unique_lock<std::mutex> lk(mu_);
        pending_.push_back(&job);
        cv_.notify_all();
        while (!job.launch) {
            if (leader_active_) { cv_.wait(lk); continue; }
            leader_active_ = true;
            // gather the announced calls, for at most a tenth of this job's chain time (half a second at most)
            const auto deadline = std::chrono::steady_clock::now() +
                                  std::chrono::microseconds((long long)(std::min(0.5, 0.1 * job.seconds) * 1e6));
            cv_.wait_until(lk, deadline, [&] { return expected_ == 0; });
            // a free lane (the pending list keeps growing meanwhile)
            int lane = -1;
            for (;;) {
                for (int i = 0; i < kHubLanes && lane < 0; ++i) {
                    Lane& l = lanes_[(next_lane_ + i) % kHubLanes];
                    if (!l.last || !l.last->done || l.last->rc != kOk || hipEventQuery(l.last->done) == hipSuccess)
                        lane = (next_lane_ + i) % kHubLanes;
                }
                if (lane >= 0) break;
                (void)hipGetLastError();   // hipErrorNotReady is not an error
                cv_.wait_for(lk, std::chrono::milliseconds(1));
            }
            next_lane_ = (lane + 1) % kHubLanes;
            // everything pending of this job's kind, this job first, up to the merged-launch limit
            std::vector<HubJob*> take{&job};
            size_t total = job.chains();
            for (HubJob* j : pending_)
                if (j != &job && j->encode == job.encode && total + j->chains() <= (size_t)kHubMaxMerged) { take.push_back(j); total += j->chains(); }
            for (HubJob* j : take) pending_.erase(std::find(pending_.begin(), pending_.end(), j));
            auto L = std::make_shared<HubLaunch>();
            lanes_[lane].last = L;
            lk.unlock();
            try {
                launch(*L, take, lanes_[lane].st, job.encode, total);
            } catch (const std::exception& e) {   // host allocation failure while merging the descriptors
                L->rc = kOutOfMemory; L->msg = std::string("merged chain launch: ") + e.what();
            }
            if (debug_on()) {
                static const auto t0 = std::chrono::steady_clock::now();
                fprintf(stderr, "[alice] hub: t=%.3f s, %s launch of %zu calls, %zu chains, lane %d\n",
                        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), job.encode ? "encode" : "decode",
                        take.size(), total, lane);
            }
            lk.lock();
            for (HubJob* j : take) j->launch = L;
            leader_active_ = false;
            cv_.notify_all();
        }
        std::shared_ptr<HubLaunch> L = job.launch;
        lk.unlock();
        if (L->rc != kOk) return fail(L->rc, L->msg);
        HIP_TRY(hipEventSynchronize(L->done));
        cv_.notify_all();   // a lane has come free
        return kOk;
    }

private:
    struct Lane { hipStream_t st = nullptr; std::shared_ptr<HubLaunch> last; };
    static void launch(HubLaunch& L, const std::vector<HubJob*>& take, hipStream_t st, bool encode, size_t total) {
        auto bad = [&](hipError_t e, const char* what) {
            if (e == hipSuccess || L.rc != kOk) return;
            L.rc = e == hipErrorOutOfMemory ? (int)kOutOfMemory : (int)kDeviceError;
            L.msg = std::string(what) + ": " + hipGetErrorString(e);
        };
        bad(hipEventCreateWithFlags(&L.done, hipEventDisableTiming), "hipEventCreate");
        size_t bytes = 0;
        const void* host = nullptr;
        if (encode) {
            L.enc.reserve(total);
            for (HubJob* j : take) L.enc.insert(L.enc.end(), j->enc.begin(), j->enc.end());
            bytes = L.enc.size() * sizeof(RansEncodeDesc); host = L.enc.data();
        } else {
            L.dec.reserve(total);
            for (HubJob* j : take) L.dec.insert(L.dec.end(), j->dec.begin(), j->dec.end());
            bytes = L.dec.size() * sizeof(RansDecodeDesc); host = L.dec.data();
        }
        if (L.rc == kOk && L.descs.alloc(bytes) != kOk) { L.rc = kOutOfMemory; L.msg = "descriptor buffer of a merged chain launch"; }
        L.descs.st = nullptr;   // every member waits for `done` before the launch object dies: nothing to drain then
        if (L.rc != kOk) return;
        for (HubJob* j : take) bad(hipStreamWaitEvent(st, j->ready, 0), "hipStreamWaitEvent");
        bad(hipMemcpyAsync(L.descs.p, host, bytes, hipMemcpyHostToDevice, st), "hipMemcpyAsync(descriptors)");
        if (L.rc != kOk) return;
        if (encode) launch_rans_encode_descs(L.descs.as<RansEncodeDesc>(), (int)total, st);
        else launch_rans_decode(L.descs.as<RansDecodeDesc>(), nullptr, (int)total, st);
        bad(hipGetLastError(), "chain launch");
        bad(hipEventRecord(L.done, st), "hipEventRecord");
    }

    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<HubJob*> pending_;
    int expected_ = 0;
    bool leader_active_ = false;
    bool ok_ = true;
    std::mutex adm_mu_;
    std::condition_variable adm_cv_;
    size_t in_flight_ = 0, budget_ = 0;   // bytes; the budget is re-measured whenever a call enters an idle hub
    bool budget_fixed_ = false;           // set by the test hook
    uint64_t next_turn_ = 0, serving_ = 0;
    int next_lane_ = 0;
    hipStream_t short_[kHubShort] = {nullptr};
    Lane lanes_[kHubLanes];
};

// A whole-chunk host call between its entry and the moment its chains are handed over: the hub's leader waits for it.
struct HubTicket {
    ChainHub* hub = nullptr;
    bool counted = false;
    hipStream_t st = nullptr;
    size_t admitted = 0;
    // device_bytes: what the call is about to allocate on the device, roughly (see ChainHub::admit)
    int open(size_t device_bytes) {
        TRY(get_stream(&st));
        hub = ChainHub::of_device(tl_device);
        hub->admit(device_bytes);
        admitted = device_bytes;
        hub->announce();
        counted = true;
        return kOk;
    }
    void arrived() { if (counted) { counted = false; hub->arrived_or_gone(); } }
    ~HubTicket() { arrived(); if (hub) hub->leave(admitted); tl_scope_stream = nullptr; }
};
// device memory of an encode / a decode of n chunks of shape d (inputs or pixels, symbols, .alc at a byte per symbol, the
// transform scratch): the figure admission works with
size_t encode_device_bytes(const ChunkDims& d, uint64_t n) { return (size_t)(n * (d.n_pixels * 3 + d.padded * 6) + forward_scratch_bytes(d)); }
// Band slot of a decode group whose chunks share one ring: every chunk's inverse plans its bands by its OWN sample width
// (launch_inverse_transform*: plan_bands at 2 or 4 bytes), the two plans cut a chunk differently, and either slot can be the
// larger (256 x 256 x 16 at a 4 MiB target: i16 6 291 712, i32 3 539 200).  any16 / any32: which widths occur in the group.
// A group of one width gets exactly that width's slot.
size_t group_scratch_bytes(const ChunkDims& d, bool any16, bool any32) {
    if (any16 && any32) return std::max(inverse_scratch_bytes(d, true), inverse_scratch_bytes(d, false));
    return inverse_scratch_bytes(d, !any32);
}
size_t decode_device_bytes(const ChunkDims& d, uint64_t n, uint64_t payload) {
    return (size_t)(n * (d.n_pixels * 3 + d.padded * 3) + payload + group_scratch_bytes(d, true, true));
}

// alice_codec_test_set_group_chunks: cap on the chunks a call works on at a time (split_group, chunks_that_fit); 0 = none.
// Host side only, read at call time.
static std::atomic<uint32_t> g_group_chunks_cap{0};
inline uint32_t cap_group(uint32_t n) {
    const uint32_t cap = g_group_chunks_cap.load(std::memory_order_relaxed);
    return cap && cap < n ? cap : n;
}

// Large device-to-host copies into the caller's pageable memory.  hipMemcpyAsync to pageable memory goes through the
// runtime's own staging at about 3 GB/s and keeps the stream busy meanwhile (110 MB of .alc: 37 ms; 64 threads' decoded
// chunks, 25 GB, over three shared streams: most of the call).  Here the copy lands in two pinned pieces of this thread,
// alternately, at the rate of the link, and the calling thread moves each piece on while the next one is in flight -- so
// the threads' CPU copies run side by side and the stream carries only the DMA.  Synchronous: returns when dst is filled.
constexpr size_t kStagePiece = size_t(32) << 20;
struct HostStage {
    void* piece[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    int device = -1;
    bool ready() {
        if (piece[0] && device == tl_device) return true;
        release();
        for (int i = 0; i < 2; ++i)
            if (hipHostMalloc(&piece[i], kStagePiece, hipHostMallocDefault) != hipSuccess ||
                hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); release(); return false; }
        device = tl_device;
        return true;
    }
    void release() {
        for (int i = 0; i < 2; ++i) {
            if (piece[i]) (void)hipHostFree(piece[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
            piece[i] = nullptr; ev[i] = nullptr;
        }
    }
    ~HostStage() { release(); }
};
thread_local HostStage tl_stage;

int copy_to_host(void* dst, const void* d_src, size_t bytes, hipStream_t st) {
    if (bytes < (size_t(4) << 20) || !tl_stage.ready()) {
        HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return kOk;
    }
    const size_t n = (bytes + kStagePiece - 1) / kStagePiece;
    auto len = [&](size_t k) { return std::min(kStagePiece, bytes - k * kStagePiece); };
    for (size_t k = 0; k <= n; ++k) {
        if (k < n) {
            HIP_TRY(hipMemcpyAsync(tl_stage.piece[k & 1], (const uint8_t*)d_src + k * kStagePiece, len(k), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipEventRecord(tl_stage.ev[k & 1], st));
        }
        if (k >= 1) {
            HIP_TRY(hipEventSynchronize(tl_stage.ev[(k - 1) & 1]));
            memcpy((uint8_t*)dst + (k - 1) * kStagePiece, tl_stage.piece[(k - 1) & 1], len(k - 1));
        }
    }
    return kOk;
}

// fn(t) on T new threads, thread t with a clean error state and device_of(t) as its device (fn calls ensure_device).
// Returns the first failure, with its message, as this thread's error.
template <typename Dev, typename Fn>
int on_threads(uint32_t T, Dev device_of, Fn fn) {
    std::vector<int> code(T, kOk);
    std::vector<std::string> msg(T);
    std::vector<std::thread> th;
    th.reserve(T);
    for (uint32_t t = 0; t < T; ++t)
        th.emplace_back([&, t] {
            clear_error();
            tl_device = device_of(t);
            code[t] = fn(t);
            if (code[t] != kOk) msg[t] = tl_msg;
        });
    for (auto& t : th) t.join();
    for (uint32_t t = 0; t < T; ++t)
        if (code[t] != kOk) return fail(code[t], msg[t]);
    return kOk;
}

// fn(i) for i in [0, n) on up to `width` helper threads bound to the calling thread's device (the copies of a many-chunk
// call: every helper moves its chunks through pinned pieces of its own, so the CPU side of the copies runs side by side).
template <typename Fn>
int parallel_chunks(uint32_t n, uint32_t width, Fn fn) {
    if (n <= 1 || width <= 1) {
        for (uint32_t i = 0; i < n; ++i) TRY(fn(i));
        return kOk;
    }
    const int device = tl_device;
    std::atomic<uint32_t> next{0};
    return on_threads(std::min(width, n), [&](uint32_t) { return device; }, [&](uint32_t) {
        TRY(ensure_device());
        for (uint32_t i; (i = next.fetch_add(1u)) < n;) TRY(fn(i));
        return (int)kOk;
    });
}
constexpr uint32_t kCopyThreads = 8;

// Every host entry point works on a short stream of its device's hub: the library owns kHubShort + kHubLanes streams per
// device and none per calling thread.
int get_stream(hipStream_t* out) {
    TRY(ensure_device());
    ChainHub* hub = ChainHub::of_device(tl_device);
    if (!hub->ok()) return fail(kDeviceError, "the streams of the chain hub could not be created");
    *out = hub->short_stream();
    tl_scope_stream = *out;
    return kOk;
}

// Hands a call's chains to the hub's next merged launch and returns when they have run; `st`: the short stream the call's
// other work is on (the chains' inputs are complete at this point of it).  Whole-chunk calls pass their ticket; the chains
// of the stage-level calls may run for seconds too, so they also leave with the merged launches instead of sitting on `st`.
int hub_chains(hipStream_t st, std::vector<RansEncodeDesc>&& enc, std::vector<RansDecodeDesc>&& dec, uint64_t symbols_per_chain,
               HubTicket* t = nullptr) {
    HubJob job;
    job.encode = !enc.empty();
    job.enc = std::move(enc);
    job.dec = std::move(dec);
    job.seconds = (double)symbols_per_chain * (job.encode ? 21e-9 : 39e-9);
    HIP_TRY(hipEventCreateWithFlags(&job.ready, hipEventDisableTiming));
    int rc = kOk;
    if (hipEventRecord(job.ready, st) != hipSuccess) rc = fail(kDeviceError, "hipEventRecord failed");
    if (t) t->arrived();
    if (rc == kOk) rc = (t ? t->hub : ChainHub::of_device(tl_device))->run(job);
    (void)hipEventDestroy(job.ready);
    return rc;
}

// ------------------------------------------------------------------------------------------
// chunk object and .alc (de)serialisation
// ------------------------------------------------------------------------------------------

struct ChannelHeader {            // reference src/pipeline.rs:123-134
    uint32_t compressed_len = 0;
    int32_t quant_step = 1;
    int32_t quant_dead_zone = 1;
    uint32_t num_symbols = 0;
    uint32_t histogram[256] = {0};
};

}  // namespace

struct EncodedChunk {             // reference src/pipeline.rs:172-185
    uint32_t width = 0, height = 0, frames = 0;
    uint8_t wavelet = kCdf53;
    ChannelHeader ch[3];
    std::vector<uint8_t> data;    // Y || Co || Cg streams
};
struct FrameEncoder { uint8_t quality; uint8_t wavelet; };
struct Wavelet1D { int kind; };
struct FastQuantizer { uint64_t reciprocal; uint32_t shift; int32_t step; int32_t dead_zone; };
// RansEncoder (src/rans.rs:238-242: state + output vector).  Every call emits its bytes back to front, so a call's
// segment reads front to back in the order finish() wants; finish() = state bytes, then the segments newest first.
struct AliceRansEncoder { uint32_t state = alice::kRansL; std::vector<std::vector<uint8_t>> segments; uint64_t bytes = 0; };
// RansDecoder (src/rans.rs:321-326: state, input, pos)
struct AliceRansDecoder;   // (defined below DevBuf: the object keeps its device copy of the input between calls)

namespace {

inline void put_u32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
inline uint32_t get_u32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// src/pipeline.rs:200-226
void chunk_to_bytes(const EncodedChunk& c, std::vector<uint8_t>& out) {
    out.resize((size_t)kAlcHeaderBytes + c.data.size());
    uint8_t* p = out.data();
    memcpy(p, "ALCC", 4);
    p[4] = 1;
    p[5] = c.wavelet;
    put_u32(p + 6, c.width); put_u32(p + 10, c.height); put_u32(p + 14, c.frames);
    size_t off = kFixedHeaderBytes;
    for (int k = 0; k < 3; ++k) {
        put_u32(p + off, c.ch[k].compressed_len); off += 4;
        put_u32(p + off, (uint32_t)c.ch[k].quant_step); off += 4;
        put_u32(p + off, (uint32_t)c.ch[k].quant_dead_zone); off += 4;
        put_u32(p + off, c.ch[k].num_symbols); off += 4;
        for (int i = 0; i < 256; ++i) { put_u32(p + off, c.ch[k].histogram[i]); off += 4; }
    }
    if (!c.data.empty()) memcpy(p + off, c.data.data(), c.data.size());
}

// header part of src/pipeline.rs:235-313; *payload_len = sum of compressed_len
int parse_alc_header(const uint8_t* data, uint64_t len, EncodedChunk& c, uint64_t* payload_len) {
    if (len < kAlcHeaderBytes)
        return fail(kInvalidBitstream, "data too short: " + std::to_string(len) + " bytes (minimum 3138)");
    if (memcmp(data, "ALCC", 4) != 0) return fail(kInvalidBitstream, "bad magic (expected ALCC)");
    if (data[4] != 1) return fail(kInvalidBitstream, "unsupported version: " + std::to_string((int)data[4]) + " (expected 1)");
    if (data[5] > 2) return fail(kInvalidBitstream, "unknown wavelet type byte: " + std::to_string((int)data[5]));
    c.wavelet = data[5];
    c.width = get_u32(data + 6); c.height = get_u32(data + 10); c.frames = get_u32(data + 14);
    size_t off = kFixedHeaderBytes;
    uint64_t total = 0;
    for (int k = 0; k < 3; ++k) {
        c.ch[k].compressed_len = get_u32(data + off); off += 4;
        c.ch[k].quant_step = (int32_t)get_u32(data + off); off += 4;
        c.ch[k].quant_dead_zone = (int32_t)get_u32(data + off); off += 4;
        c.ch[k].num_symbols = get_u32(data + off); off += 4;
        for (int i = 0; i < 256; ++i) { c.ch[k].histogram[i] = get_u32(data + off); off += 4; }
        total += c.ch[k].compressed_len;
    }
    *payload_len = total;
    return kOk;
}

int chunk_from_bytes(const uint8_t* data, uint64_t len, EncodedChunk& c) {
    uint64_t total = 0;
    TRY(parse_alc_header(data, len, c, &total));
    if (len < (uint64_t)kAlcHeaderBytes + total)
        return fail(kInvalidBitstream, "truncated payload: need " + std::to_string(kAlcHeaderBytes + total - len) + " more bytes");
    c.data.assign(data + kAlcHeaderBytes, data + kAlcHeaderBytes + total);
    return kOk;
}

// src/pipeline.rs:67-71
int checked_pixel_count(uint64_t w, uint64_t h, uint64_t f, uint64_t* out) {
    unsigned __int128 v = (unsigned __int128)w * h;
    if (v > UINT64_MAX) return fail(kDimensionOverflow, "dimensions overflow usize");
    v *= f;
    if (v > UINT64_MAX) return fail(kDimensionOverflow, "dimensions overflow usize");
    *out = (uint64_t)v;
    return kOk;
}

// The shape checks of the calls outside the reference: a pixel count that fits, a non-empty chunk (and `count` chunks of
// it: a batch of none is empty too), a padded volume the header's u32 num_symbols can count.
int chunk_dims(uint32_t w, uint32_t h, uint32_t f, ChunkDims* d, uint32_t count = 1) {
    uint64_t n_pixels = 0;
    TRY(checked_pixel_count(w, h, f, &n_pixels));
    if (n_pixels == 0 || count == 0) return fail(kInvalidDimensions, count ? "invalid dimensions" : "empty batch");
    *d = make_dims(w, h, f);
    if (d->padded > 0xFFFFFFFFull) return fail(kDimensionOverflow, "padded pixel count does not fit the header's u32 num_symbols");
    return kOk;
}

// ------------------------------------------------------------------------------------------
// encode / decode on device buffers
// ------------------------------------------------------------------------------------------

inline uint64_t round_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// Rigorous magnitude bound through the inverse 3-D lifting.  max_q bounds |q|: symbols of versions 1 and 2 are u8, so
// |q| <= 128 (kByteMaxQ); a version 3 stream decodes to z <= 255 + 4095, so |q| <= 2175 (kWideMaxQ).  Every
// dequantised sample is at most max_q * |step|; each lifting step adds at most (2 * other * |c| + 4096) / 8192 + 1.
// The flags of launch_inverse_transform: exact unless 32-bit (24 x 24-bit) products are exact everywhere; mid16 (never with
// exact): every value after the temporal pass fits i16, so it can be stored in 16 bits; lds16: also after the column pass.
// The same bound covers the mirrored inverse of version 4: its step subtracts
// floor((v + 4096) / 8192) with v = (a + b) * c, and |floor((v + 4096) / 8192)| <= (|v| + 4096) / 8192 + 1 is the increment
// above; the operand and product conditions of the 24-bit multiply depend on |a + b| and |c| only.
struct InverseBounds { bool exact; bool mid16; bool lds16; };

// The container of the lane-parallel orchestration (PART 4): version 2 (u8 symbols), version 3 (u16 symbols, the
// reference's inverse) or version 4 (version 3 with the mirrored inverse).  Wide and reversible size and launch alike
// except for the version byte and the inverse launcher.
enum SplitFormat : int { kFormatSplit = 0, kFormatWide = 1, kFormatReversible = 2 };
inline bool is_wide(SplitFormat f) { return f != kFormatSplit; }
inline uint8_t format_version(SplitFormat f) { return (uint8_t)(2 + (int)f); }
inline SplitFormat format_of_version(int version) { return version == 4 ? kFormatReversible : version == 3 ? kFormatWide : kFormatSplit; }
constexpr int kByteMaxQ = 128;
InverseBounds inverse_bounds(int wavelet, const int32_t step[3], int max_q = kByteMaxQ) {
    const LiftSteps ls = lift_steps(wavelet);
    long double worst = 0;
    for (int c = 0; c < 3; ++c) {
        long double a = (long double)max_q * fabsl((long double)step[c]);
        if (a > worst) worst = a;
    }
    const InverseBounds exact{true, false, false};
    InverseBounds r{false, false, false};
    long double m = worst;  // bound on every sample
    for (int pass = 0; pass < 3; ++pass) {
        long double me = m, mo = m;
        for (int k = ls.n - 1; k >= 0; --k) {
            const long double cabs = fabsl((long double)ls.coeff[k]);
            long double& target = (k & 1) == 0 ? mo : me;
            const long double other = (k & 1) == 0 ? me : mo;
            // v_mul_i24 operands: |a + b| < 2^23; product + rounding below 2^31
            if (2 * other >= 8388607.0L || 2 * other * cabs + 4096 >= 2147483647.0L) return exact;
            target = target + (2 * other * cabs + 4096) / 8192 + 1;
            if (target >= 1073741824.0L) return exact;
        }
        m = me > mo ? me : mo;
        if (pass == 0) r.mid16 = m <= 32767.0L;
        if (pass == 1) r.lds16 = r.mid16 && m <= 32767.0L;
    }
    return r;
}

struct EncodeWork {
    ChunkDims d{};
    int n_chunks = 0;
    uint64_t cap[3] = {0, 0, 0}, alc_stride = 0;   // stream regions of the Y, Co, Cg chains of a chunk
    DevBuf scratch;   // band slots of the tile path (forward_scratch_bytes; a batch sizes it for its decode side too)
    DevBuf gen, tmp, sym, hist, tables, results, alc, sizes, planes;   // gen / tmp / planes: generic path only
};

int encode_work_alloc(EncodeWork& w, const ChunkDims& d, int n_chunks, size_t scratch_bytes = 0) {
    w.d = d; w.n_chunks = n_chunks; w.cap[0] = w.cap[1] = w.cap[2] = 0; w.alc_stride = 0;
    if (transform_tiles_eligible(d)) TRY(w.scratch.alloc(std::max(forward_scratch_bytes(d), scratch_bytes)));
    TRY(w.sym.alloc((size_t)n_chunks * 3 * d.padded));
    TRY(w.hist.alloc((size_t)n_chunks * 3 * 256 * sizeof(uint32_t)));
    TRY(w.tables.alloc((size_t)n_chunks * 3 * sizeof(RansTable)));
    TRY(w.results.alloc((size_t)n_chunks * 3 * sizeof(RansResult)));
    TRY(w.sizes.alloc((size_t)n_chunks * sizeof(unsigned long long)));
    return kOk;
}

// .alc buffers for the capacities of the three chains of a chunk (re-allocated only when one grows).  A chunk's buffer is
// [kStreamHead bytes][region Y][region Co][region Cg]: the chains write their streams at the tails of their regions and
// the compaction moves them, in place, behind the header at the front.
int encode_work_set_cap(EncodeWork& w, const uint64_t cap[3]) {
    if (w.alc.p && cap[0] <= w.cap[0] && cap[1] <= w.cap[1] && cap[2] <= w.cap[2]) return kOk;
    w.alc.reset();
    for (int c = 0; c < 3; ++c) w.cap[c] = std::max(w.cap[c], cap[c]);
    w.alc_stride = round_up(kStreamHead + w.cap[0] + w.cap[1] + w.cap[2], 256);
    TRY(w.alc.alloc((size_t)w.n_chunks * w.alc_stride + 256));  // slack: the compaction copy reads whole dwords
    return kOk;
}

// Upper bound of a chain's stream length from its histogram.  The table is the reference's
// (src/rans.rs:102-150); a symbol of frequency f costs log2(4096 / f) bits, the floor in x / f loses less
// than log2(1 + 2^-11) bits per symbol (the state is at least f * 2^11 when it is divided), and the final
// state adds 4 bytes.  A margin on top keeps this a capacity, not a prediction; the kernel still checks.
uint64_t estimate_stream_cap(const uint32_t* hist, uint64_t n) {
    unsigned long long total = 0;
    for (int i = 0; i < 256; ++i) total += hist[i];
    if (total == 0) return 4096;
    long double bits = 0;
    unsigned nt = 0;
    unsigned freq[256];
    for (int i = 0; i < 256; ++i) {
        unsigned f = hist[i] == 0 ? 1u : (unsigned)std::max<unsigned long long>((unsigned long long)hist[i] * kProbScale / total, 1ull);
        freq[i] = f;
        nt += f;
    }
    if (nt != kProbScale) freq[255] = (unsigned)((int)freq[255] + ((int)kProbScale - (int)nt)) & 0xFFFFu;
    for (int i = 0; i < 256; ++i) {
        if (!hist[i]) continue;
        const unsigned f = freq[i];
        if (f == 0) return 0;                                   // reported by the kernel as a divergence
        if (f < kProbScale) bits += (long double)hist[i] * log2l((long double)kProbScale / (long double)f);
    }
    const long double bytes = bits / 8.0L;
    return (uint64_t)(bytes * 1.002L) + n / 4096 + 4096 + 64;
}

uint64_t worst_cap(const ChunkDims& d) { return round_up(2 * d.padded + 4 + 64 + 64, 256); }  // +64: dummy-store guard band

// The generic path's forward transform of one chunk: exact reference arithmetic on caller-shaped data (chunks of more than 64
// padded frames, say); per_channel(c, vol) gets each channel's coefficient volume (d.padded i32, followed by as much room).
template <typename Fn>
int generic_forward(const RgbLayout& rgb, const ChunkDims& d, int wavelet, EncodeWork& w, hipStream_t st, Fn per_channel) {
    if (!w.planes.p) TRY(w.planes.alloc(3 * d.n_pixels * sizeof(int16_t)));
    if (!w.tmp.p) TRY(w.tmp.alloc(d.padded * sizeof(int32_t)));
    if (!w.gen.p) TRY(w.gen.alloc(2 * d.padded * sizeof(int32_t)));
    int16_t* pl = w.planes.as<int16_t>();
    launch_rgb_to_ycocg(rgb, d, pl, pl + d.n_pixels, pl + 2 * d.n_pixels, st);
    int32_t* vol = w.gen.as<int32_t>();
    const uint64_t W = d.pw, H = d.ph, D = d.pf;
    for (int c = 0; c < 3; ++c) {
        launch_pad_channel(pl + (size_t)c * d.n_pixels, d, vol, st);
        launch_wavelet_axis(vol, w.tmp.as<int32_t>(), W, 1, D * H, W, 1, 0, wavelet, false, st);
        launch_wavelet_axis(vol, w.tmp.as<int32_t>(), H, W, D, W * H, W, 1, wavelet, false, st);
        launch_wavelet_axis(vol, w.tmp.as<int32_t>(), D, W * H, 1, 0, W * H, 1, wavelet, false, st);
        per_channel(c, vol);
    }
    return kOk;
}

// The forward transform of one chunk: the tile kernels where they cover the shape (w.scratch holds their band slots), else
// the generic path.
// wide: d_sym holds 3 * d.padded untruncated u16 symbols (.alc v3) and the histogram bins min(z, 255).
int forward_chunk(const RgbLayout& rgb, const ChunkDims& d, int wavelet, int32_t step, EncodeWork& w,
                  uint8_t* d_sym, uint32_t* d_hist, hipStream_t st, bool wide = false) {
    if (wide) {
        uint16_t* zs = (uint16_t*)d_sym;
        if (w.scratch.p && launch_forward_transform_wide(rgb, d, wavelet, step, w.scratch.p, zs, d_hist, st)) return kOk;
        return generic_forward(rgb, d, wavelet, w, st, [&](int c, int32_t* vol) {
            int32_t* qb = vol + d.padded;
            launch_quantize(vol, qb, d.padded, step, step, st);
            launch_to_symbols_wide(qb, zs + (size_t)c * d.padded, d.padded, st);
            launch_histogram_wide(zs + (size_t)c * d.padded, d.padded, d_hist + c * 256, st);
        });
    }
    if (w.scratch.p && launch_forward_transform(rgb, d, wavelet, step, w.scratch.p, d_sym, d_hist, st)) return kOk;
    return generic_forward(rgb, d, wavelet, w, st, [&](int c, int32_t* vol) {
        int32_t* qb = vol + d.padded;
        launch_quantize(vol, qb, d.padded, step, step, st);
        launch_to_symbols(qb, d_sym + (size_t)c * d.padded, d.padded, st);
        launch_histogram(d_sym + (size_t)c * d.padded, d.padded, d_hist + c * 256, st);
    });
}

// ---- rate prediction (rate.hip) ----
constexpr int kQualities = 101;

// Coefficient bins of one chunk (bins: [3][4096], zeroed; oor: the chunk's out-of-range counter, zeroed).
int coef_hist_chunk(const RgbLayout& rgb, const ChunkDims& d, int wavelet, EncodeWork& w, uint32_t* d_bins, uint32_t* d_oor,
                    hipStream_t st) {
    if (w.scratch.p && launch_forward_coef_hist(rgb, d, wavelet, w.scratch.p, d_bins, d_oor, st)) return kOk;
    return generic_forward(rgb, d, wavelet, w, st, [&](int c, int32_t* vol) { launch_coef_hist(vol, d.padded, d_bins + (size_t)c * 4096, d_oor, st); });
}

// Stream-length brackets of n chunks at every step: out[(chunk * 64 + step - 1) * 3 + channel].  w: the chunk shape's
// forward scratch (EncodeWork of one chunk).  d_step_hist: [chunk][step - 1][channel][256] u32 on the device, or null.
// A chunk with coefficients outside the value table's range (never for 8-bit RGB at the default radius) gets its step
// histograms from the real forward pass at each of the 64 steps instead of the fold.  split_lane != 0: the brackets are
// those of the split-stream channel payloads at that lane_symbols (rate.hip, split_cost_kernel) instead of the v1 streams.
// wide (with split_lane): the wide container's -- the histograms are of the coded symbol min(z, 255) (fold_kernel<true>, and
// the wide forward pass with its 2-byte symbols in the fallback) and the brackets are wide_cost_kernel's.
// Returns after the stream has drained.
int predict_chunks(const RgbLayout* rgb, uint32_t n, const ChunkDims& d, int wavelet, EncodeWork& w, hipStream_t st,
                   uint32_t* d_step_hist, std::vector<RateChannel>& out, uint32_t split_lane = 0, bool wide = false) {
    const size_t per_chunk = (size_t)64 * 3;
    DevBuf bins, oor, own_hist, res, logt, fsym;
    TRY(bins.alloc((size_t)n * 3 * 4096 * sizeof(uint32_t)));
    TRY(oor.alloc((size_t)n * sizeof(uint32_t)));
    TRY(res.alloc((size_t)n * per_chunk * sizeof(RateChannel)));
    TRY(logt.alloc(2 * (kProbScale + 1) * sizeof(uint32_t)));
    if (!d_step_hist) { TRY(own_hist.alloc((size_t)n * per_chunk * 256 * sizeof(uint32_t))); d_step_hist = own_hist.as<uint32_t>(); }
    const RateLogTable& t = rate_log_table();
    HIP_TRY(hipMemcpyAsync(logt.p, t.lo, sizeof(t.lo), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(logt.as<uint32_t>() + (kProbScale + 1), t.hi, sizeof(t.hi), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(bins.p, 0, (size_t)n * 3 * 4096 * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(oor.p, 0, (size_t)n * sizeof(uint32_t), st));
    for (uint32_t b = 0; b < n; ++b)
        TRY(coef_hist_chunk(rgb[b], d, wavelet, w, bins.as<uint32_t>() + (size_t)b * 3 * 4096, oor.as<uint32_t>() + b, st));
    if (wide) launch_rate_fold_wide(bins.as<uint32_t>(), oor.as<uint32_t>(), n, d_step_hist, st);
    else launch_rate_fold(bins.as<uint32_t>(), oor.as<uint32_t>(), n, d_step_hist, st);
    std::vector<uint32_t> h_oor(n);
    HIP_TRY(hipMemcpyAsync(h_oor.data(), oor.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t b = 0; b < n; ++b) {
        if (!h_oor[b]) continue;
        if (!fsym.p) TRY(fsym.alloc(3 * d.padded * (wide ? 2 : 1)));   // (not w.sym: a batch keeps its decoded pixels there)
        for (int32_t step = 1; step <= 64; ++step) {
            uint32_t* h = d_step_hist + ((size_t)b * 64 + (size_t)(step - 1)) * 3 * 256;
            HIP_TRY(hipMemsetAsync(h, 0, 3 * 256 * sizeof(uint32_t), st));
            TRY(forward_chunk(rgb[b], d, wavelet, step, w, fsym.as<uint8_t>(), h, st, wide));
        }
    }
    if (wide) launch_wide_rate_cost(d_step_hist, logt.as<uint32_t>(), n, split_lane, res.as<RateChannel>(), st);
    else if (split_lane) launch_split_rate_cost(d_step_hist, logt.as<uint32_t>(), n, split_lane, res.as<RateChannel>(), st);
    else launch_rate_cost(d_step_hist, logt.as<uint32_t>(), n, res.as<RateChannel>(), st);
    HIP_TRY(hipGetLastError());
    out.resize((size_t)n * per_chunk);
    HIP_TRY(hipMemcpyAsync(out.data(), res.p, out.size() * sizeof(RateChannel), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}

// Whole-.alc brackets of one chunk at the 101 qualities from its 64 x 3 channel brackets: 3138 + the three streams, or
// lo = 0, hi = UINT64_MAX and the worst channel status when a channel's table is not bounded.
void rate_by_quality(const RateChannel* rc, uint64_t* lo, uint64_t* hi, uint8_t* status) {
    for (int q = 0; q < kQualities; ++q) {
        const RateChannel* c = rc + (size_t)(quality_to_step((uint8_t)q) - 1) * 3;
        const uint32_t worst = std::max(c[0].status, std::max(c[1].status, c[2].status));
        status[q] = (uint8_t)worst;
        lo[q] = worst == kRateBounded ? kAlcHeaderBytes + c[0].lo + c[1].lo + c[2].lo : 0;
        hi[q] = worst == kRateBounded ? kAlcHeaderBytes + c[0].hi + c[1].hi + c[2].hi : UINT64_MAX;
    }
}

// An empty chunk (no pixels) is its header alone at every quality.
void rate_of_empty_chunk(uint64_t* lo, uint64_t* hi, uint8_t* status) {
    for (int q = 0; q < kQualities; ++q) { lo[q] = hi[q] = kAlcHeaderBytes; status[q] = (uint8_t)kRateBounded; }
}

// The budget rule: the largest quality in [min_q, max_q] whose prediction is bounded and whose upper bound fits the budget
// (every quality is looked at: size need not fall with quality); min_q with *fits = 0 when none does.  Qualities above 100
// act as 100.
uint8_t choose_quality(const uint64_t* hi, const uint8_t* status, uint64_t budget, uint8_t min_q, uint8_t max_q, uint8_t* fits) {
    min_q = std::min<uint8_t>(min_q, 100); max_q = std::min<uint8_t>(max_q, 100);
    for (int q = max_q; q >= min_q; --q)
        if (status[q] == kRateBounded && hi[q] <= budget) { *fits = 1; return (uint8_t)q; }
    *fits = 0;
    return min_q;
}

thread_local uint64_t tl_test_first_cap = 0;   // alice_codec_test_force_first_cap
thread_local uint32_t tl_dec_stats[4] = {0, 0, 0, 0};   // last single-chain decode of this thread: fast tiles, exact tiles, path mask, bytes consumed
void note_decode_stats(const RansResult& r) {
    tl_dec_stats[0] = r.fast_tiles; tl_dec_stats[1] = r.slow_tiles; tl_dec_stats[2] = r.paths;
    tl_dec_stats[3] = (uint32_t)(r.len > 0xFFFFFFFFull ? 0xFFFFFFFFull : r.len);
}

struct StageEvents {
    hipEvent_t ev[8] = {nullptr};
    bool ready = false;
    int init() {
        if (ready) return kOk;
        for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
        ready = true;
        return kOk;
    }
    ~StageEvents() { if (ready) for (auto& e : ev) (void)hipEventDestroy(e); }
};

// Encode of n_chunks chunks on `st`; results stay on the device.  How the stream regions are sized:
//   kCapReuse    the work area already owns .alc buffers (a batch after its first encode): keep their capacities and
//                queue everything without touching the host -- the chains check their regions, and a chunk that outgrew
//                them (new content) comes back as an overflow, which the caller answers with kCapEstimate;
//   kCapEstimate one host round trip between the transforms and the chains reads the histograms and derives a capacity
//                per channel (estimate_stream_cap); also what kCapReuse falls back to when there are no buffers yet;
//   kCapWorst    2 bytes per symbol, the bound of the format (the last resort: 3 x 2 x padded bytes per chunk).
enum CapMode { kCapReuse = 0, kCapEstimate = 1, kCapWorst = 2 };
// rgb[b]: where chunk b's pixels are (w.n_chunks layouts)
// qualities: one per chunk (alice_codec_batch_set_qualities), or null for `quality` everywhere
int encode_launch(const RgbLayout* rgb, EncodeWork& w, uint8_t quality, int wavelet, hipStream_t st,
                  StageEvents* evs, CapMode mode = kCapReuse, HubTicket* hub = nullptr, const uint8_t* qualities = nullptr) {
    const ChunkDims& d = w.d;
    const int32_t step = quality_to_step(quality);
    const int B = w.n_chunks;
    HIP_TRY(hipMemsetAsync(w.hist.p, 0, (size_t)B * 3 * 256 * sizeof(uint32_t), st));
    if (evs) HIP_TRY(hipEventRecord(evs->ev[0], st));
    for (int b = 0; b < B; ++b) {
        uint8_t* sym = w.sym.as<uint8_t>() + (size_t)b * 3 * d.padded;
        TRY(forward_chunk(rgb[b], d, wavelet, qualities ? quality_to_step(qualities[b]) : step, w, sym,
                          w.hist.as<uint32_t>() + (size_t)b * 3 * 256, st));
    }
    if (evs) HIP_TRY(hipEventRecord(evs->ev[1], st));
    const bool had_alc = w.alc.p != nullptr;
    uint64_t cap[3] = {w.cap[0], w.cap[1], w.cap[2]};
    if (mode == kCapWorst) {
        cap[0] = cap[1] = cap[2] = worst_cap(d);
    } else if (mode == kCapEstimate || !had_alc) {
        cap[0] = cap[1] = cap[2] = 0;
        std::vector<uint32_t> hist((size_t)B * 3 * 256);
        HIP_TRY(hipMemcpyAsync(hist.data(), w.hist.p, hist.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        // one capacity per channel (the largest over the chunks): Y streams are about twice as long as Co / Cg streams
        for (int c = 0; c < 3 * B; ++c) cap[c % 3] = std::max(cap[c % 3], estimate_stream_cap(&hist[(size_t)c * 256], d.padded));
        for (int c = 0; c < 3; ++c) cap[c] = std::min(round_up(cap[c], 256), worst_cap(d));
        // test-only override (alice_codec_test_force_first_cap): pretend the first estimate was far too small, to
        // exercise the overflow-and-retry path
        if (mode == kCapReuse && !had_alc)
            if (const uint64_t forced = tl_test_first_cap) cap[0] = cap[1] = cap[2] = forced;
    }
    TRY(encode_work_set_cap(w, cap));
    launch_rans_table(w.hist.as<uint32_t>(), w.tables.as<RansTable>(), 3 * B, st);
    if (evs) HIP_TRY(hipEventRecord(evs->ev[2], st));
    if (hub) {
        // host call: the chains leave with the hub's next merged launch (same regions as the grouped layout below); this
        // thread sleeps until they have run and then queues the tail on its short stream
        std::vector<RansEncodeDesc> enc((size_t)3 * B);
        for (int c = 0; c < 3 * B; ++c) {
            RansEncodeDesc& e = enc[(size_t)c];
            const int g = c % 3;
            e.sym = w.sym.as<uint8_t>() + (size_t)c * d.padded;
            e.n = d.padded;
            e.table = w.tables.as<RansTable>() + c;
            e.region = w.alc.as<uint8_t>() + (size_t)(c / 3) * w.alc_stride + kStreamHead + (g == 0 ? 0ull : (g == 1 ? w.cap[0] : w.cap[0] + w.cap[1]));
            e.cap = w.cap[g];
            e.result = w.results.as<RansResult>() + c;
            e.x_init = kRansL;
            e.keep_open = 0u;
        }
        TRY(hub_chains(st, std::move(enc), {}, d.padded, hub));
    } else {
        launch_rans_encode(w.sym.as<uint8_t>(), d.padded, d.padded, w.tables.as<RansTable>(), w.alc.as<uint8_t>(),
                           w.cap[0], w.results.as<RansResult>(), 3 * B, st, w.alc_stride, kStreamHead, 0xFFFFFFFFu, w.cap[1], w.cap[2]);
    }
    if (evs) HIP_TRY(hipEventRecord(evs->ev[3], st));
    if (!qualities)
        launch_write_headers(w.alc.as<uint8_t>(), w.alc_stride, d, wavelet, step, w.hist.as<uint32_t>(),
                             w.results.as<RansResult>(), w.sizes.as<unsigned long long>(), B, st);
    else   // each chunk's header carries its own step
        for (int b = 0; b < B; ++b)
            launch_write_headers(w.alc.as<uint8_t>() + (size_t)b * w.alc_stride, w.alc_stride, d, wavelet, quality_to_step(qualities[b]),
                                 w.hist.as<uint32_t>() + (size_t)b * 3 * 256, w.results.as<RansResult>() + 3 * b,
                                 w.sizes.as<unsigned long long>() + b, 1, st);
    launch_compact_streams(w.alc.as<uint8_t>(), w.alc_stride, kStreamHead, w.cap, w.results.as<RansResult>(), B, st);
    if (evs) HIP_TRY(hipEventRecord(evs->ev[4], st));
    HIP_TRY(hipGetLastError());
    return kOk;
}

// The error an encode chain's flags report, overflow aside: what that means is the caller's.
int encode_flags_error(uint32_t flags) {
    if (flags & kTableDiverges)
        return fail(kReferenceDiverges, "a symbol whose table frequency wrapped to 0 is present: the reference encoder does not terminate on this input");
    if (flags & kRansInternal) return fail(kInternal, "rANS kernel invariant violated");
    return kOk;
}

constexpr int kOverflowed = -1;   // encode_collect: a chain outgrew its stream region, encode again with more room

// After the stream has drained: fetch per-chain results, map flags to errors.
int encode_collect(EncodeWork& w, hipStream_t st, std::vector<RansResult>& res) {
    res.resize((size_t)w.n_chunks * 3);
    HIP_TRY(hipMemcpyAsync(res.data(), w.results.p, res.size() * sizeof(RansResult), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (auto& r : res) TRY(encode_flags_error(r.flags));
    if (debug_on())
        for (size_t i = 0; i < res.size(); ++i)
            fprintf(stderr, "[alice] encode chain %zu: %llu bytes, %.1f Mcycles, %.1f ms of 100 MHz ticks => %.2f GHz, xcc %u se %u cu %u simd %u\n", i, res[i].len,
                    res[i].cycles_k * 1024.0 / 1e6, res[i].ticks_k * 1024.0 / 1e5,
                    res[i].ticks_k ? (res[i].cycles_k / (double)res[i].ticks_k) * 0.1 : 0.0,
                    res[i].xcc_id & 15u, (res[i].hw_id >> 13) & 7u, (res[i].hw_id >> 8) & 15u, (res[i].hw_id >> 4) & 3u);
    for (auto& r : res)
        if (r.flags & kRansOverflow) return kOverflowed;
    return kOk;
}

// The capacity ladder: encodes from `mode` on, one CapMode further after every overflow.  kCapWorst is the format's bound,
// so a chain that overflows even there is an internal error.
int encode_with_retry(const RgbLayout* rgb, EncodeWork& w, uint8_t quality, int wavelet, hipStream_t st, StageEvents* evs,
                      CapMode mode, HubTicket* hub, std::vector<RansResult>& res, const uint8_t* qualities = nullptr) {
    for (int m = mode; m <= kCapWorst; ++m) {
        TRY(encode_launch(rgb, w, quality, wavelet, st, evs, (CapMode)m, hub, qualities));
        const int rc = encode_collect(w, st, res);
        if (rc != kOverflowed) return rc;
    }
    return fail(kInternal, "rANS output exceeded the worst-case capacity");
}

struct DecodeWork {
    ChunkDims d{};
    int n_chunks = 0;
    DevBuf scratch_own, gen, tmp, sym, hist, tables, descs, results, planes;
    uint8_t* sym_ptr = nullptr;   // decoded symbols: own buffer, or one lent by the caller
    DevBuf* scratch = nullptr;    // band slots of the tile path: own buffer, or the one a batch shares with its encode side
};

// sym_ext / scratch_ext: buffers the caller lends (a batch reuses its encode-side symbol and scratch buffers,
// which are dead once the encode has finished)
int decode_work_alloc(DecodeWork& w, const ChunkDims& d, int n_chunks, uint8_t* sym_ext = nullptr, DevBuf* scratch_ext = nullptr) {
    w.d = d; w.n_chunks = n_chunks;
    w.scratch = scratch_ext ? scratch_ext : &w.scratch_own;
    if (sym_ext) w.sym_ptr = sym_ext;
    else { TRY(w.sym.alloc((size_t)n_chunks * 3 * d.padded)); w.sym_ptr = w.sym.as<uint8_t>(); }
    TRY(w.hist.alloc((size_t)n_chunks * 3 * 256 * sizeof(uint32_t)));
    TRY(w.tables.alloc((size_t)n_chunks * 3 * sizeof(RansTable)));
    TRY(w.descs.alloc((size_t)n_chunks * 3 * sizeof(RansDecodeDesc)));
    TRY(w.results.alloc((size_t)n_chunks * 3 * sizeof(RansResult)));
    return kOk;
}

// The inverse transform of one chunk: the tile kernels where they cover the shape (d_scratch: their band slots, null when
// they do not), else exact reference arithmetic.
// fmt wide or reversible: d_sym holds u16 symbols (.alc v3, v4), and the instance choice starts from |q| <= kWideMaxQ;
// reversible: every lifting step is the forward's mirror (the tile kernels' MIRROR instances, the generic path's mirror mode).
int inverse_chunk(const uint8_t* d_sym, const ChunkDims& d, int wavelet, const int32_t step[3], void* d_scratch, DecodeWork& w,
                  const RgbLayout& rgb, hipStream_t st, SplitFormat fmt = kFormatSplit) {
    const bool wide = is_wide(fmt), mirror = fmt == kFormatReversible;
    const InverseBounds ib = inverse_bounds(wavelet, step, wide ? kWideMaxQ : kByteMaxQ);
    if (mirror) {
        if (d_scratch && launch_inverse_transform_reversible((const uint16_t*)d_sym, d, wavelet, step, ib.exact, ib.mid16, ib.lds16, d_scratch, rgb, st))
            return kOk;
    } else if (wide) {
        if (d_scratch && launch_inverse_transform_wide((const uint16_t*)d_sym, d, wavelet, step, ib.exact, ib.mid16, ib.lds16, d_scratch, rgb, st))
            return kOk;
    } else if (d_scratch && launch_inverse_transform(d_sym, d, wavelet, step, ib.exact, ib.mid16, ib.lds16, d_scratch, rgb, st)) return kOk;
    if (!w.planes.p) TRY(w.planes.alloc(3 * d.n_pixels * sizeof(int16_t)));
    if (!w.tmp.p) TRY(w.tmp.alloc(d.padded * sizeof(int32_t)));
    if (!w.gen.p) TRY(w.gen.alloc(2 * d.padded * sizeof(int32_t)));
    int16_t* pl = w.planes.as<int16_t>();
    int32_t* qb = w.gen.as<int32_t>();
    int32_t* vol = qb + d.padded;
    const uint64_t W = d.pw, H = d.ph, D = d.pf;
    for (int c = 0; c < 3; ++c) {
        if (wide) launch_from_symbols_wide((const uint16_t*)d_sym + (size_t)c * d.padded, qb, d.padded, st);
        else launch_from_symbols(d_sym + (size_t)c * d.padded, qb, d.padded, st);
        launch_dequantize(qb, vol, d.padded, step[c], st);
        launch_wavelet_axis(vol, w.tmp.as<int32_t>(), D, W * H, 1, 0, W * H, 1, wavelet, true, st, mirror);
        launch_wavelet_axis(vol, w.tmp.as<int32_t>(), H, W, D, W * H, W, 1, wavelet, true, st, mirror);
        launch_wavelet_axis(vol, w.tmp.as<int32_t>(), W, 1, D * H, W, 1, 0, wavelet, true, st, mirror);
        launch_strip_channel(vol, d, pl + (size_t)c * d.n_pixels, st);
    }
    launch_ycocg_to_rgb(pl, pl + d.n_pixels, pl + 2 * d.n_pixels, d, rgb, st);
    return kOk;
}

// headers[b]: parsed chunk headers (validated); d_payload[b]: device pointer to chunk b's payload;
// rgb[b]: where chunk b's pixels go
int decode_launch(const EncodedChunk* const* headers, const std::vector<const uint8_t*>& d_payload,
                  DecodeWork& w, const std::vector<RgbLayout>& rgb, hipStream_t st, StageEvents* evs, HubTicket* hub = nullptr) {
    const ChunkDims& d = w.d;
    const int B = w.n_chunks;
    if (transform_tiles_eligible(d)) {
        // band slots: i16 when every chunk's bound allows it, else i32 (sized before anything is queued: the chunks of
        // a batch share the ring, and growing it must not wait for the chains)
        bool any16 = false, any32 = false;
        for (int b = 0; b < B; ++b) {
            const int32_t step[3] = {headers[b]->ch[0].quant_step, headers[b]->ch[1].quant_step, headers[b]->ch[2].quant_step};
            (inverse_bounds(headers[b]->wavelet, step).mid16 ? any16 : any32) = true;
        }
        const size_t need = group_scratch_bytes(d, any16, any32);
        if (!w.scratch->p || w.scratch->n < need) {
            HIP_TRY(hipStreamSynchronize(st));   // an earlier call's tail may still use the old ring
            TRY(w.scratch->alloc(need));
        }
    }
    std::vector<uint32_t> hist((size_t)B * 3 * 256);
    std::vector<RansDecodeDesc> descs((size_t)B * 3);
    for (int b = 0; b < B; ++b) {
        uint64_t off = 0;
        for (int c = 0; c < 3; ++c) {
            const ChannelHeader& h = headers[b]->ch[c];
            memcpy(&hist[((size_t)b * 3 + c) * 256], h.histogram, 256 * sizeof(uint32_t));
            RansDecodeDesc& ds = descs[(size_t)b * 3 + c];
            ds.in = d_payload[b] + off;
            ds.in_len = h.compressed_len;
            ds.out = w.sym_ptr + ((size_t)b * 3 + c) * d.padded;
            ds.n = d.padded;
            ds.table = w.tables.as<RansTable>() + ((size_t)b * 3 + c);
            off += h.compressed_len;
        }
    }
    HIP_TRY(hipMemcpyAsync(w.hist.p, hist.data(), hist.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (!hub) HIP_TRY(hipMemcpyAsync(w.descs.p, descs.data(), descs.size() * sizeof(RansDecodeDesc), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // host vectors go out of scope
    if (evs) HIP_TRY(hipEventRecord(evs->ev[5], st));
    launch_rans_table(w.hist.as<uint32_t>(), w.tables.as<RansTable>(), 3 * B, st);
    if (hub) {   // host call: see encode_launch
        for (size_t c = 0; c < descs.size(); ++c) descs[c].result = w.results.as<RansResult>() + c;
        TRY(hub_chains(st, {}, std::move(descs), d.padded, hub));
    } else {
        launch_rans_decode(w.descs.as<RansDecodeDesc>(), w.results.as<RansResult>(), 3 * B, st);
    }
    if (evs) HIP_TRY(hipEventRecord(evs->ev[6], st));
    for (int b = 0; b < B; ++b) {
        const int32_t step[3] = {headers[b]->ch[0].quant_step, headers[b]->ch[1].quant_step, headers[b]->ch[2].quant_step};
        TRY(inverse_chunk(w.sym_ptr + (size_t)b * 3 * d.padded, d, headers[b]->wavelet, step, w.scratch->p, w, rgb[b], st));
    }
    if (evs) HIP_TRY(hipEventRecord(evs->ev[7], st));
    HIP_TRY(hipGetLastError());
    return kOk;
}

int decode_collect(DecodeWork& w, hipStream_t st) {
    std::vector<RansResult> res((size_t)w.n_chunks * 3);
    HIP_TRY(hipMemcpyAsync(res.data(), w.results.p, res.size() * sizeof(RansResult), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (auto& r : res)
        if (r.flags & kRansInternal) return fail(kInternal, "rANS decode table invariant violated");
    if (debug_on())
        for (size_t i = 0; i < res.size(); ++i)
            fprintf(stderr, "[alice] decode chain %zu: consumed %llu bytes, fast tiles %u, slow tiles %u, %.1f Mcycles, xcc %u se %u cu %u simd %u\n", i, res[i].len,
                    res[i].fast_tiles, res[i].slow_tiles, res[i].cycles_k * 1024.0 / 1e6,
                    res[i].xcc_id & 15u, (res[i].hw_id >> 13) & 7u, (res[i].hw_id >> 8) & 15u, (res[i].hw_id >> 4) & 3u);
    return kOk;
}

// src/pipeline.rs:537-579 validation, in the reference's order
int validate_for_decode(const EncodedChunk& c, ChunkDims* dims, uint64_t payload_len) {
    uint64_t n_pixels = 0;
    TRY(checked_pixel_count(c.width, c.height, c.frames, &n_pixels));
    *dims = make_dims(c.width, c.height, c.frames);
    if (n_pixels == 0) return kOk;
    uint64_t off = 0;
    for (int k = 0; k < 3; ++k) {
        if ((uint64_t)c.ch[k].num_symbols != dims->padded)
            return fail(kInvalidBitstream, "channel " + std::to_string(k) + ": num_symbols " + std::to_string(c.ch[k].num_symbols) +
                                               " != padded_pixels " + std::to_string(dims->padded));
        if (off + c.ch[k].compressed_len > payload_len)
            return fail(kInvalidBitstream, "channel " + std::to_string(k) + ": compressed data overrun");
        off += c.ch[k].compressed_len;
    }
    return kOk;
}

// How many chunks of this shape the calling thread's device can hold at once (inputs or outputs, symbols, .alc
// buffers with the worst observed payload of 1 byte per pixel sample, tables), leaving a fifth of the free memory alone.
uint32_t chunks_that_fit(const ChunkDims& d, uint32_t want) {
    if (want <= 1) return want;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return cap_group(want); }
    const long double per_chunk = (long double)d.n_pixels * 3 + (long double)d.padded * 3 * 2 + 3.0L * sizeof(RansTable) * 2 + 65536;
    const long double fixed = (long double)std::max(forward_scratch_bytes(d), group_scratch_bytes(d, true, true)) + (64u << 20);
    const long double room = (long double)free_b * 0.8L - fixed;
    if (room < per_chunk) return 1;
    const long double n = room / per_chunk;
    return cap_group(n >= (long double)want ? want : (uint32_t)n);
}

// The n_chunks encoded chunks of w (chain results res) as chunk objects: chunk i's object goes to slot(i) (left for the
// caller to delete on error).  All headers with one strided copy, then the payloads straight into the objects, several at
// a time.
template <typename Slot>
int chunks_to_host(EncodeWork& w, const std::vector<RansResult>& res, hipStream_t st, Slot slot) {
    const uint32_t B = (uint32_t)w.n_chunks;
    std::vector<uint8_t> hdr((size_t)B * kAlcHeaderBytes);
    if (hipMemcpy2DAsync(hdr.data(), kAlcHeaderBytes, w.alc.p, w.alc_stride, kAlcHeaderBytes, B, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(kDeviceError, "device to host copy failed");
    return parallel_chunks(B, w.alc_stride >= (4u << 20) ? kCopyThreads : 1u, [&](uint32_t i) {
        const uint64_t payload = res[3 * i].len + res[3 * i + 1].len + res[3 * i + 2].len;
        EncodedChunk* c = slot(i) = new (std::nothrow) EncodedChunk();
        if (!c) return fail(kOutOfMemory, "out of host memory");
        uint64_t tot = 0;
        if (parse_alc_header(hdr.data() + (size_t)i * kAlcHeaderBytes, kAlcHeaderBytes + payload, *c, &tot) != kOk || tot != payload)
            return fail(kInternal, "device header/payload length mismatch");
        c->data.resize((size_t)payload);
        return copy_to_host(c->data.data(), w.alc.as<uint8_t>() + (size_t)i * w.alc_stride + kAlcHeaderBytes, (size_t)payload, st);
    });
}

// The quality range of a budget call, after qualities above 100 have become 100.
int check_quality_range(uint8_t min_q, uint8_t max_q) {
    if (std::min<uint8_t>(min_q, 100) > std::min<uint8_t>(max_q, 100)) return fail(kInvalidDimensions, "min_quality > max_quality");
    return kOk;
}

// Every whole-chunk encode from host memory: chunks k = slot, slot + step, ... below n_chunks of rgb (n_pixels * 3 bytes
// each) on the calling thread's device, as many at a time as its memory holds, into out[k].  On error nothing is left in
// out.  One chunk is the case n = 1 (parallel_chunks then runs its copies inline).
int encode_chunks_on_device(const FrameEncoder& enc, const uint8_t* rgb, const ChunkDims& d, EncodedChunk** out, uint32_t n_chunks,
                            uint32_t slot = 0, uint32_t step = 1) {
    const uint32_t n = slot < n_chunks ? (n_chunks - slot + step - 1) / step : 0;
    auto at = [&](uint32_t i) { return slot + (size_t)i * step; };   // this call's i-th chunk
    for (uint32_t i = 0; i < n; ++i) out[at(i)] = nullptr;
    if (!n) return kOk;
    TRY(ensure_device());
    const uint32_t per_pass = chunks_that_fit(d, n);
    HubTicket ticket;
    TRY(ticket.open(encode_device_bytes(d, per_pass)));
    const hipStream_t st = ticket.st;
    auto undo = [&](int rc) { for (uint32_t i = 0; i < n; ++i) { delete out[at(i)]; out[at(i)] = nullptr; } return rc; };
    const uint64_t chunk_bytes = d.n_pixels * 3;
    for (uint32_t first = 0; first < n; first += per_pass) {
        const uint32_t B = std::min(per_pass, n - first);
        DevBuf d_rgb;
        EncodeWork w;
        std::vector<RansResult> res;
        int rc = d_rgb.alloc(chunk_bytes * B);
        if (rc == kOk) rc = encode_work_alloc(w, d, (int)B);
        if (rc == kOk)
            rc = parallel_chunks(B, chunk_bytes >= (4u << 20) ? kCopyThreads : 1u, [&](uint32_t i) {
                HIP_TRY(hipMemcpyAsync(d_rgb.as<uint8_t>() + (size_t)i * chunk_bytes, rgb + at(first + i) * chunk_bytes, chunk_bytes, hipMemcpyHostToDevice, st));
                return (int)kOk;
            });
        std::vector<RgbLayout> layouts(B);
        for (uint32_t i = 0; i < B; ++i) layouts[i] = packed_rgb(d_rgb.as<uint8_t>() + (size_t)i * chunk_bytes, d);
        if (rc == kOk) rc = encode_with_retry(layouts.data(), w, enc.quality, enc.wavelet, st, nullptr, kCapReuse, &ticket, res);
        if (rc == kOk) rc = chunks_to_host(w, res, st, [&](uint32_t i) -> EncodedChunk*& { return out[at(first + i)]; });
        if (rc != kOk) return undo(rc);
    }
    return kOk;
}

// Every whole-chunk decode into host memory, chunks chosen as by encode_chunks_on_device (all of one shape, validated by the
// caller): chunk k's pixels go to rgb_out + k * n_pixels * 3.  Empty chunks return before any device is touched.
int decode_chunks_on_device(const EncodedChunk* const* chunks, const ChunkDims& d, uint8_t* rgb_out, uint32_t n_chunks,
                            uint32_t slot = 0, uint32_t step = 1) {
    const uint32_t n = slot < n_chunks ? (n_chunks - slot + step - 1) / step : 0;
    auto at = [&](uint32_t i) { return slot + (size_t)i * step; };
    if (!n || d.n_pixels == 0) return kOk;
    TRY(ensure_device());
    const uint32_t per_pass = chunks_that_fit(d, n);
    uint64_t max_payload = 0;
    for (uint32_t i = 0; i < n; ++i) max_payload = std::max<uint64_t>(max_payload, chunks[at(i)]->data.size());
    HubTicket ticket;
    TRY(ticket.open(decode_device_bytes(d, per_pass, (uint64_t)per_pass * (max_payload + 512))));
    const hipStream_t st = ticket.st;
    const uint64_t chunk_bytes = d.n_pixels * 3;
    for (uint32_t first = 0; first < n; first += per_pass) {
        const uint32_t B = std::min(per_pass, n - first);
        std::vector<const EncodedChunk*> hdrs(B);
        uint64_t total_payload = 0;
        for (uint32_t i = 0; i < B; ++i) { hdrs[i] = chunks[at(first + i)]; total_payload += round_up(hdrs[i]->data.size() + 16, 256); }
        DevBuf d_payload, d_rgb;
        TRY(d_payload.alloc(total_payload + 256));
        TRY(d_rgb.alloc(chunk_bytes * B));
        std::vector<const uint8_t*> pay(B);
        std::vector<RgbLayout> dst(B);
        uint64_t off = 0;
        for (uint32_t i = 0; i < B; ++i) {
            const EncodedChunk& c = *hdrs[i];
            pay[i] = d_payload.as<uint8_t>() + off;
            dst[i] = packed_rgb(d_rgb.as<uint8_t>() + (size_t)i * chunk_bytes, d);
            if (!c.data.empty())
                HIP_TRY(hipMemcpyAsync(d_payload.as<uint8_t>() + off, c.data.data(), c.data.size(), hipMemcpyHostToDevice, st));
            off += round_up(c.data.size() + 16, 256);
        }
        DecodeWork w;
        TRY(decode_work_alloc(w, d, (int)B));
        TRY(decode_launch(hdrs.data(), pay, w, dst, st, nullptr, &ticket));
        TRY(decode_collect(w, st));
        TRY(parallel_chunks(B, chunk_bytes >= (4u << 20) ? kCopyThreads : 1u,
                            [&](uint32_t i) { return copy_to_host(rgb_out + at(first + i) * chunk_bytes, dst[i].base, chunk_bytes, st); }));
    }
    return kOk;
}

// FrameEncoder::encode's validation (src/pipeline.rs:388-427, in its order) of n_chunks chunks in one buffer: the checks of
// one chunk, with the buffer n_chunks times as long.  The calls of one chunk answer the empty chunk (:391-412) before.
int validate_encode_many(const FrameEncoder* encoder, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                         uint32_t frames, uint32_t n_chunks, EncodedChunk** out_chunks, ChunkDims* d) {
    if (!encoder || !out_chunks || (!rgb && rgb_len)) return fail(kNullArgument, "null argument");
    for (uint32_t i = 0; i < n_chunks; ++i) out_chunks[i] = nullptr;
    if (n_chunks == 0) return kOk;
    uint64_t n_pixels = 0;
    TRY(checked_pixel_count(width, height, frames, &n_pixels));                             // :388
    if (n_pixels == 0 || width == 0 || height == 0) return fail(kInvalidDimensions, "invalid dimensions");   // :415-417
    if (n_pixels > UINT64_MAX / 3 / n_chunks) return fail(kDimensionOverflow, "dimensions overflow usize");
    if (rgb_len != n_pixels * 3 * n_chunks)                                                 // :422-427
        return fail(kInvalidBufferSize, "buffer size mismatch: expected " + std::to_string(n_pixels * 3 * n_chunks) + ", got " + std::to_string(rgb_len));
    return chunk_dims(width, height, frames, d);
}

// FrameEncoder::encode on host buffers (src/pipeline.rs:377-507); *out: the chunk object
int encode_host(const FrameEncoder& enc, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                uint32_t frames, EncodedChunk** out) {
    uint64_t n_pixels = 0;
    TRY(checked_pixel_count(width, height, frames, &n_pixels));                 // :388
    if (n_pixels == 0) {                                                         // :391-412
        if (rgb_len != 0) return fail(kInvalidBufferSize, "buffer size mismatch: expected 0, got " + std::to_string(rgb_len));
        *out = new (std::nothrow) EncodedChunk{width, height, frames, enc.wavelet};
        return *out ? kOk : fail(kOutOfMemory, "out of host memory");
    }
    ChunkDims d{};
    TRY(validate_encode_many(&enc, rgb, rgb_len, width, height, frames, 1, out, &d));
    return encode_chunks_on_device(enc, rgb, d, out, 1);
}

// FrameEncoder::encode of one host chunk at the highest quality in [min_q, max_q] whose predicted size fits max_bytes (see
// choose_quality): one upload, the prediction, one encode, on the hub's path like every whole-chunk host call.
int encode_to_size_host(uint8_t wavelet, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height, uint32_t frames,
                        uint64_t max_bytes, uint8_t min_q, uint8_t max_q, uint8_t* chosen, uint8_t* fits, EncodedChunk** out) {
    uint64_t lo[kQualities], hi[kQualities];
    uint8_t status[kQualities];
    uint64_t n_pixels = 0;
    TRY(checked_pixel_count(width, height, frames, &n_pixels));                 // src/pipeline.rs:388
    if (n_pixels == 0) {                                                         // :391-412
        if (rgb_len != 0) return fail(kInvalidBufferSize, "buffer size mismatch: expected 0, got " + std::to_string(rgb_len));
        TRY(check_quality_range(min_q, max_q));
        rate_of_empty_chunk(lo, hi, status);
        *chosen = choose_quality(hi, status, max_bytes, min_q, max_q, fits);
        *out = new (std::nothrow) EncodedChunk{width, height, frames, wavelet};
        return *out ? kOk : fail(kOutOfMemory, "out of host memory");
    }
    const FrameEncoder enc{0, wavelet};
    ChunkDims d{};
    TRY(validate_encode_many(&enc, rgb, rgb_len, width, height, frames, 1, out, &d));
    TRY(check_quality_range(min_q, max_q));
    TRY(ensure_device());
    HubTicket ticket;
    TRY(ticket.open(encode_device_bytes(d, 1)));
    const hipStream_t st = ticket.st;
    DevBuf d_rgb;
    EncodeWork w;
    TRY(d_rgb.alloc(n_pixels * 3));
    TRY(encode_work_alloc(w, d, 1));
    HIP_TRY(hipMemcpyAsync(d_rgb.p, rgb, n_pixels * 3, hipMemcpyHostToDevice, st));
    const RgbLayout layout = packed_rgb(d_rgb.as<uint8_t>(), d);
    std::vector<RateChannel> rc;
    TRY(predict_chunks(&layout, 1, d, wavelet, w, st, nullptr, rc));
    rate_by_quality(rc.data(), lo, hi, status);
    *chosen = choose_quality(hi, status, max_bytes, min_q, max_q, fits);
    std::vector<RansResult> res;
    TRY(encode_with_retry(&layout, w, *chosen, wavelet, st, nullptr, kCapReuse, &ticket, res));
    const int r = chunks_to_host(w, res, st, [&](uint32_t) -> EncodedChunk*& { return *out; });
    if (r != kOk) { delete *out; *out = nullptr; }
    return r;
}

// The prediction of one host chunk (alice_codec_predict_sizes): one upload on a short stream of the hub; no chains, so the
// call leaves the hub's gathering at once.
int predict_sizes_host(uint8_t wavelet, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height, uint32_t frames,
                       uint64_t* lo, uint64_t* hi, uint8_t* status) {
    uint64_t n_pixels = 0;
    TRY(checked_pixel_count(width, height, frames, &n_pixels));                 // src/pipeline.rs:388
    if (n_pixels == 0) {                                                         // :391-412
        if (rgb_len != 0) return fail(kInvalidBufferSize, "buffer size mismatch: expected 0, got " + std::to_string(rgb_len));
        rate_of_empty_chunk(lo, hi, status);
        return kOk;
    }
    const FrameEncoder enc{0, wavelet};
    EncodedChunk* none = nullptr;
    ChunkDims d{};
    TRY(validate_encode_many(&enc, rgb, rgb_len, width, height, frames, 1, &none, &d));
    TRY(ensure_device());
    HubTicket ticket;
    TRY(ticket.open(encode_device_bytes(d, 1)));
    ticket.arrived();
    DevBuf d_rgb;
    EncodeWork w;
    w.d = d; w.n_chunks = 1;
    if (transform_tiles_eligible(d)) TRY(w.scratch.alloc(forward_scratch_bytes(d)));
    TRY(d_rgb.alloc(n_pixels * 3));
    HIP_TRY(hipMemcpyAsync(d_rgb.p, rgb, n_pixels * 3, hipMemcpyHostToDevice, ticket.st));
    const RgbLayout layout = packed_rgb(d_rgb.as<uint8_t>(), d);
    std::vector<RateChannel> rc;
    TRY(predict_chunks(&layout, 1, d, wavelet, w, ticket.st, nullptr, rc));
    rate_by_quality(rc.data(), lo, hi, status);
    return kOk;
}

// A buffer the C ABI hands to the caller (released with free(): alice_codec_data_free64).  Large ones are 2 MiB aligned and
// marked for huge pages: 64 threads that each fault a fresh 398 MB result in 4 KiB pages spend more time in the kernel's
// page-fault path than the GPU spends on their chains.
uint8_t* host_result_alloc(uint64_t bytes) {
    constexpr size_t kHuge = size_t(2) << 20;
    if (bytes < 2 * kHuge) return (uint8_t*)malloc(bytes ? (size_t)bytes : 1);
    const size_t len = round_up(bytes, kHuge);
    void* p = aligned_alloc(kHuge, len);
    if (p) (void)madvise(p, len, MADV_HUGEPAGE);
    return (uint8_t*)p;
}

// FrameDecoder::decode on a host chunk (src/pipeline.rs:537-624): *out receives malloc'ed pixels, *out_len their count
int decode_host(const EncodedChunk& c, uint8_t** out, uint64_t* out_len) {
    ChunkDims d;
    TRY(validate_for_decode(c, &d, c.data.size()));
    *out = nullptr; *out_len = 0;
    uint8_t* rgb = host_result_alloc(d.n_pixels * 3);
    if (!rgb) return fail(kOutOfMemory, "out of host memory");
    const EncodedChunk* one = &c;
    const int rc = decode_chunks_on_device(&one, d, rgb, 1);
    if (rc != kOk) { free(rgb); return rc; }
    *out = rgb; *out_len = d.n_pixels * 3;
    return kOk;
}

uint8_t* to_c_buffer(const std::vector<uint8_t>& v) {
    uint8_t* p = (uint8_t*)malloc(v.size() ? v.size() : 1);
    if (p && !v.empty()) memcpy(p, v.data(), v.size());
    return p;
}

// generic staged run: copy in, run fn on device pointers, copy out
template <typename Tin, typename Tout, typename Fn>
int staged(const Tin* in, uint64_t n_in, Tout* out, uint64_t n_out, Fn fn) {
    hipStream_t st;
    TRY(get_stream(&st));
    DevBuf a, b;
    TRY(a.alloc(n_in * sizeof(Tin)));
    TRY(b.alloc(n_out * sizeof(Tout)));
    if (n_in) HIP_TRY(hipMemcpyAsync(a.p, in, n_in * sizeof(Tin), hipMemcpyHostToDevice, st));
    fn(a.as<Tin>(), b.as<Tout>(), st);
    HIP_TRY(hipGetLastError());
    if (n_out) HIP_TRY(hipMemcpyAsync(out, b.p, n_out * sizeof(Tout), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}

// Wavelet1D / 2D / 3D of a device-resident volume, result in `v` (tmp: same size).  Volumes the tile kernels cover run
// their exact instances (two passes over the data); the rest -- odd lengths, tiny sizes, 1-D signals -- runs the
// per-axis kernels of generic.hip.
void wavelet_on_device(int kind, int32_t* v, int32_t* tmp, uint64_t W, uint64_t H, uint64_t D, int ndim, bool inverse, hipStream_t st) {
    if (stage_tiles_eligible(W, H, D, ndim)) { launch_stage_wavelet(v, tmp, W, H, D, ndim, kind, inverse, st); return; }
    if (!inverse) {
        launch_wavelet_axis(v, tmp, W, 1, D * H, W, 1, 0, kind, false, st);
        if (ndim >= 2) launch_wavelet_axis(v, tmp, H, W, D, W * H, W, 1, kind, false, st);
        if (ndim >= 3) launch_wavelet_axis(v, tmp, D, W * H, 1, 0, W * H, 1, kind, false, st);
    } else {
        if (ndim >= 3) launch_wavelet_axis(v, tmp, D, W * H, 1, 0, W * H, 1, kind, true, st);
        if (ndim >= 2) launch_wavelet_axis(v, tmp, H, W, D, W * H, W, 1, kind, true, st);
        launch_wavelet_axis(v, tmp, W, 1, D * H, W, 1, 0, kind, true, st);
    }
}

int wavelet_nd(int kind, int32_t* data, uint64_t W, uint64_t H, uint64_t D, int ndim, bool inverse) {
    if (!data) return fail(kNullArgument, "null data");
    if (kind < 0 || kind > 2) return fail(kInvalidBitstream, "unknown wavelet type");
    unsigned __int128 tot = (unsigned __int128)W * H * D;
    if (tot > ((unsigned __int128)1 << 40)) return fail(kDimensionOverflow, "volume too large");
    const uint64_t n = (uint64_t)tot;
    if (n == 0) return kOk;
    hipStream_t st;
    TRY(get_stream(&st));
    DevBuf a, t;
    TRY(a.alloc(n * 4));
    TRY(t.alloc(n * 4));
    HIP_TRY(hipMemcpyAsync(a.p, data, n * 4, hipMemcpyHostToDevice, st));
    wavelet_on_device(kind, a.as<int32_t>(), t.as<int32_t>(), W, H, D, ndim, inverse, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(data, a.p, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}

// ---- the stage-level rANS calls: a frequency table of the caller's, one chain or the four of the interleaved format ----

// The caller's (cum_freq, freq) pair built into k identical tables on the device; buf holds the pair, then the tables.
int stage_tables(const uint16_t* cum_freq, const uint16_t* freq, int k, DevBuf& buf, hipStream_t st, RansTable** tables) {
    TRY(buf.alloc(1024 + (size_t)k * sizeof(RansTable)));
    uint16_t* arrays = buf.as<uint16_t>();
    HIP_TRY(hipMemcpyAsync(arrays, cum_freq, 512, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(arrays + 256, freq, 512, hipMemcpyHostToDevice, st));
    *tables = (RansTable*)(buf.as<uint8_t>() + 1024);
    for (int j = 0; j < k; ++j) launch_rans_table_from_arrays(arrays, arrays + 256, *tables + j, st);
    return kOk;
}

// One encode chain from state x_init (keep_open: an encoder object carries the state on, its four bytes stay unwritten);
// the stream, res.len bytes, is copied to dst(res.len), a host buffer of the caller's (null: out of memory, or 0 bytes).
template <typename Dst>
int stage_encode_chain(const uint8_t* symbols, uint64_t n, const uint16_t* cum_freq, const uint16_t* freq, uint32_t x_init,
                       uint32_t keep_open, RansResult& res, Dst dst) {
    hipStream_t st;
    TRY(get_stream(&st));
    const uint64_t cap = round_up(2 * n + 4 + 64 + 64, 256);
    DevBuf ds, dt, dout, dres;
    RansTable* table = nullptr;
    TRY(ds.alloc(n)); TRY(dout.alloc(cap)); TRY(dres.alloc(sizeof(RansResult)));
    if (n) HIP_TRY(hipMemcpyAsync(ds.p, symbols, n, hipMemcpyHostToDevice, st));
    TRY(stage_tables(cum_freq, freq, 1, dt, st, &table));
    TRY(hub_chains(st, {RansEncodeDesc{ds.as<uint8_t>(), n, table, dout.as<uint8_t>(), cap, dres.as<RansResult>(), x_init, keep_open}}, {}, n));
    HIP_TRY(hipMemcpyAsync(&res, dres.p, sizeof(res), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    TRY(encode_flags_error(res.flags));
    if (res.flags & kRansOverflow) return fail(kInternal, "rANS output exceeded the worst-case capacity");
    uint8_t* p = dst(res.len);
    if (!p && res.len) return fail(kOutOfMemory, "out of host memory");
    if (res.len) {
        HIP_TRY(hipMemcpyAsync(p, dout.as<uint8_t>() + (cap - res.len), res.len, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return kOk;
}

// One decode chain on `st`: n symbols of the stream at d_in (len bytes) into symbols[] on the host; resume: continue from
// state x0 at byte pos0, where a decoder object stopped, instead of from the stream's four head bytes.
int stage_decode_chain(hipStream_t st, const uint8_t* d_in, uint64_t len, const uint16_t* cum_freq, const uint16_t* freq, uint64_t n,
                       uint32_t resume, uint32_t x0, uint64_t pos0, uint8_t* symbols, RansResult& res) {
    DevBuf dt, dout, dres;
    RansTable* table = nullptr;
    TRY(dout.alloc(n)); TRY(dres.alloc(sizeof(RansResult)));
    TRY(stage_tables(cum_freq, freq, 1, dt, st, &table));
    TRY(hub_chains(st, {}, {RansDecodeDesc{d_in, len, dout.as<uint8_t>(), n, table, resume, x0, pos0, dres.as<RansResult>()}}, n));
    HIP_TRY(hipMemcpyAsync(&res, dres.p, sizeof(res), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(symbols, dout.p, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    note_decode_stats(res);
    if (res.flags & kRansInternal) return fail(kInternal, "rANS decode kernel invariant violated");
    return kOk;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// batches
// ------------------------------------------------------------------------------------------

struct AliceBatch {
    ChunkDims d{};
    uint32_t n_chunks = 0;
    uint8_t quality = 0, wavelet = 0;
    int device = 0;
    EncodeWork enc;
    DecodeWork dec;
    DevBuf spare;             // in-place decode: the pixels of chunk 0 (chunk i > 0 lands on the symbols of chunk i - 1)
    std::vector<RgbLayout> rgb_dst;  // where the last decode put each chunk's pixels
    bool dec_ready = false;
    StageEvents evs;
    hipStream_t enc_stream = nullptr, dec_stream = nullptr;
    std::vector<RgbLayout> last_rgb;   // where the last encode read each chunk (packed or a region): what a retry re-reads
    std::vector<uint8_t> qualities;    // one per chunk (alice_codec_batch_set_qualities); empty: `quality` for every chunk
    const uint8_t* chunk_qualities() const { return qualities.empty() ? nullptr : qualities.data(); }
    bool enc_timed = false, dec_timed = false;
    float stage_ms[6] = {0, 0, 0, 0, 0, 0};
};

namespace {

// Chunk i of a region call: frames [i * f, (i + 1) * f) of the frame_width x frame_height frames at d_frames (packed RGB),
// cropped to the batch's w x h at origins[2i], origins[2i + 1].  Every rectangle must lie inside the frame: where the
// reference's crop_to_bbox / paste_from_bbox skip rows that fall outside (src/segment.rs:275-276, 293), this is an error
// before anything is queued.
int region_layouts(const AliceBatch* b, const void* d_frames, uint32_t frame_width, uint32_t frame_height, const uint32_t* origins,
                   std::vector<RgbLayout>& out) {
    if (!b || !d_frames || !origins) return fail(kNullArgument, "null argument");
    uint64_t frame_px = 0;
    TRY(checked_pixel_count(frame_width, frame_height, (uint64_t)b->d.f * b->n_chunks, &frame_px));
    if (frame_px > UINT64_MAX / 3) return fail(kDimensionOverflow, "dimensions overflow usize");
    const uint64_t row_pitch = 3ull * frame_width, frame_pitch = row_pitch * frame_height;
    out.resize(b->n_chunks);
    for (uint32_t i = 0; i < b->n_chunks; ++i) {
        const uint64_t x0 = origins[2 * i], y0 = origins[2 * i + 1];
        if (x0 + b->d.w > frame_width || y0 + b->d.h > frame_height)
            return fail(kInvalidDimensions, "region " + std::to_string(i) + " at (" + std::to_string(x0) + ", " + std::to_string(y0) +
                                                ") does not lie inside the " + std::to_string(frame_width) + "x" + std::to_string(frame_height) + " frame");
        out[i] = RgbLayout{(uint8_t*)d_frames + (size_t)i * b->d.f * frame_pitch + y0 * row_pitch + x0 * 3, row_pitch, frame_pitch};
    }
    return kOk;
}

// rgb: one layout per chunk, kept for encode_finish's retry
int batch_encode_layouts(AliceBatch* b, std::vector<RgbLayout>&& rgb, hipStream_t st) {
    DeviceScope ds(b->device);
    if (!ds.ok) return tl_err;
    tl_scope_stream = nullptr;   // batch buffers outlive the call; alice_codec_batch_destroy drains the device
    b->enc_stream = st;
    b->enc_timed = false;
    b->last_rgb = std::move(rgb);
    return encode_launch(b->last_rgb.data(), b->enc, b->quality, b->wavelet, b->enc_stream, &b->evs, kCapReuse, nullptr,
                         b->chunk_qualities());
}

// rgb: one layout per chunk, or empty for the batch's own storage
int batch_decode_layouts(AliceBatch* b, const void* d_alc, uint64_t alc_stride, std::vector<RgbLayout>&& rgb, hipStream_t st) {
    DeviceScope ds(b->device);
    if (!ds.ok) return tl_err;
    tl_scope_stream = nullptr;
    b->dec_stream = st;
    b->dec_timed = false;
    if (!b->dec_ready) {
        TRY(decode_work_alloc(b->dec, b->d, (int)b->n_chunks, b->enc.sym.as<uint8_t>(), &b->enc.scratch));
        b->dec_ready = true;
    }
    // headers: one strided device-to-host copy, then validation on the host
    std::vector<uint8_t> hdr((size_t)b->n_chunks * kAlcHeaderBytes);
    HIP_TRY(hipMemcpy2DAsync(hdr.data(), kAlcHeaderBytes, d_alc, alc_stride, kAlcHeaderBytes, b->n_chunks, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<EncodedChunk> headers(b->n_chunks);
    std::vector<const EncodedChunk*> hp(b->n_chunks);
    std::vector<const uint8_t*> pay(b->n_chunks);
    for (uint32_t i = 0; i < b->n_chunks; ++i) {
        uint64_t payload = 0;
        TRY(parse_alc_header(hdr.data() + (size_t)i * kAlcHeaderBytes, kAlcHeaderBytes, headers[i], &payload));
        if (headers[i].width != b->d.w || headers[i].height != b->d.h || headers[i].frames != b->d.f)
            return fail(kInvalidDimensions, "chunk dimensions differ from the batch shape");
        if ((uint64_t)kAlcHeaderBytes + payload > alc_stride) return fail(kInvalidBitstream, "truncated payload");
        ChunkDims dd;
        TRY(validate_for_decode(headers[i], &dd, payload));
        pay[i] = (const uint8_t*)d_alc + (size_t)i * alc_stride + kAlcHeaderBytes;
        hp[i] = &headers[i];
    }
    // no layouts: the batch keeps the pixels in its own storage (alice_codec_batch_rgb_ptr).  An uncut chunk is
    // reconstructed over its own (by then consumed) symbols: its temporal pass is the last reader of those symbols and
    // runs before the tile pass that writes the pixels.  A chunk that is cut into bands writes the pixels of its first
    // band while the temporal pass of its later bands still reads symbols: the pixels of chunk i then land on the symbols
    // of chunk i - 1, whose last reader finished launches ago, and chunk 0 gets a buffer of its own.
    if (rgb.empty()) {
        const bool cut = inverse_cuts_chunk(b->d);
        if (cut && !b->spare.p) TRY(b->spare.alloc(b->d.n_pixels * 3));
        rgb.resize(b->n_chunks);
        for (uint32_t i = 0; i < b->n_chunks; ++i)
            rgb[i] = packed_rgb(!cut ? b->dec.sym_ptr + (size_t)i * 3 * b->d.padded
                                     : (i == 0 ? b->spare.as<uint8_t>() : b->dec.sym_ptr + (size_t)(i - 1) * 3 * b->d.padded), b->d);
    }
    b->rgb_dst = std::move(rgb);
    return decode_launch(hp.data(), pay, b->dec, b->rgb_dst, st, &b->evs);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------

extern "C" {

// ---- PART 1: reference ABI ----

Wavelet1D* alice_codec_wavelet1d_haar(void) { return new (std::nothrow) Wavelet1D{kHaar}; }
Wavelet1D* alice_codec_wavelet1d_cdf53(void) { return new (std::nothrow) Wavelet1D{kCdf53}; }
Wavelet1D* alice_codec_wavelet1d_cdf97(void) { return new (std::nothrow) Wavelet1D{kCdf97}; }
void alice_codec_wavelet1d_destroy(Wavelet1D* ptr) { delete ptr; }

void alice_codec_wavelet1d_forward(const Wavelet1D* w, int32_t* data, uint32_t len) {
    clear_error();
    if (!w || !data || len < 2) return;
    (void)wavelet_nd(w->kind, data, len, 1, 1, 1, false);
}
void alice_codec_wavelet1d_inverse(const Wavelet1D* w, int32_t* data, uint32_t len) {
    clear_error();
    if (!w || !data || len < 2) return;
    (void)wavelet_nd(w->kind, data, len, 1, 1, 1, true);
}

FrameEncoder* alice_codec_encoder_create(uint8_t quality) { return new (std::nothrow) FrameEncoder{quality, (uint8_t)kCdf53}; }
void alice_codec_encoder_destroy(FrameEncoder* ptr) { delete ptr; }

EncodedChunk* alice_codec_encode64(const FrameEncoder* encoder, const uint8_t* rgb, uint64_t rgb_len, uint32_t width,
                                   uint32_t height, uint32_t frames) {
    clear_error();
    if (!encoder || !rgb) { fail(kNullArgument, "null argument"); return nullptr; }
    EncodedChunk* c = nullptr;
    return encode_host(*encoder, rgb, rgb_len, width, height, frames, &c) == kOk ? c : nullptr;
}
EncodedChunk* alice_codec_encode(const FrameEncoder* encoder, const uint8_t* rgb, uint32_t rgb_len, uint32_t width,
                                 uint32_t height, uint32_t frames) {
    return alice_codec_encode64(encoder, rgb, rgb_len, width, height, frames);
}

uint8_t* alice_codec_decode64(const EncodedChunk* chunk, uint64_t* out_len) {
    clear_error();
    if (!chunk || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    uint8_t* p = nullptr;
    if (decode_host(*chunk, &p, out_len) != kOk) return nullptr;
    return p;
}
uint8_t* alice_codec_decode(const EncodedChunk* chunk, uint32_t* out_len) {
    if (!chunk || !out_len) { clear_error(); fail(kNullArgument, "null argument"); return nullptr; }
    uint64_t n = 0;
    uint8_t* p = alice_codec_decode64(chunk, &n);
    if (p) *out_len = (uint32_t)n;  // `rgb.len() as u32`, src/ffi.rs:157
    return p;
}

void alice_codec_chunk_destroy(EncodedChunk* ptr) { delete ptr; }

uint8_t* alice_codec_chunk_to_bytes64(const EncodedChunk* chunk, uint64_t* out_len) {
    clear_error();
    if (!chunk || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    std::vector<uint8_t> v;
    chunk_to_bytes(*chunk, v);
    uint8_t* p = to_c_buffer(v);
    if (!p) { fail(kOutOfMemory, "out of host memory"); return nullptr; }
    *out_len = v.size();
    return p;
}
uint8_t* alice_codec_chunk_to_bytes(const EncodedChunk* chunk, uint32_t* out_len) {
    if (!chunk || !out_len) { clear_error(); fail(kNullArgument, "null argument"); return nullptr; }
    uint64_t n = 0;
    uint8_t* p = alice_codec_chunk_to_bytes64(chunk, &n);
    if (p) *out_len = (uint32_t)n;
    return p;
}
EncodedChunk* alice_codec_chunk_from_bytes64(const uint8_t* data, uint64_t len) {
    clear_error();
    if (!data) { fail(kNullArgument, "null argument"); return nullptr; }
    EncodedChunk* c = new (std::nothrow) EncodedChunk();
    if (!c) { fail(kOutOfMemory, "out of host memory"); return nullptr; }
    if (chunk_from_bytes(data, len, *c) != kOk) { delete c; return nullptr; }
    return c;
}
EncodedChunk* alice_codec_chunk_from_bytes(const uint8_t* data, uint32_t len) { return alice_codec_chunk_from_bytes64(data, len); }

uint32_t alice_codec_chunk_width(const EncodedChunk* c) { return c ? c->width : 0; }
uint32_t alice_codec_chunk_height(const EncodedChunk* c) { return c ? c->height : 0; }
uint32_t alice_codec_chunk_frames(const EncodedChunk* c) { return c ? c->frames : 0; }

double alice_codec_psnr(const uint8_t* a, const uint8_t* b, uint32_t len) {
    clear_error();
    if (!a || !b) return -1.0;
    if (len == 0) return INFINITY;  // mse 0.0 for empty buffers (src/metrics.rs:23-25)
    hipStream_t st;
    if (get_stream(&st) != kOk) return -1.0;
    DevBuf da, db, ds;
    if (da.alloc(len) || db.alloc(len) || ds.alloc(8)) return -1.0;
    unsigned long long sum = 0;
    if (hipMemcpyAsync(da.p, a, len, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(db.p, b, len, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(ds.p, 0, 8, st) != hipSuccess) { fail(kDeviceError, "copy failed"); return -1.0; }
    launch_sq_diff_sum(da.as<uint8_t>(), db.as<uint8_t>(), len, ds.as<unsigned long long>(), st);
    if (hipMemcpyAsync(&sum, ds.p, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) { fail(kDeviceError, "psnr kernel failed"); return -1.0; }
    return alice_codec_psnr_from_sse(sum, len);   // one expression for every dB value the library reports
}

void alice_codec_data_free64(uint8_t* ptr, uint64_t len) { (void)len; if (ptr) free(ptr); }
void alice_codec_data_free(uint8_t* ptr, uint32_t len) {
    // reference: no-op when ptr is NULL or len == 0 (src/ffi.rs:289); our zero-length buffers are
    // 1-byte mallocs, released here too so nothing leaks
    (void)len;
    if (ptr) free(ptr);
}
void alice_codec_string_free(char* s) { free(s); }
char* alice_codec_version(void) {
    const char* v = "0.1.2";  // CARGO_PKG_VERSION of the reference (Cargo.toml)
    char* p = (char*)malloc(strlen(v) + 1);
    if (p) strcpy(p, v);
    return p;
}

// ---- PART 2: extensions ----

int alice_codec_last_error(void) { return tl_err; }
const char* alice_codec_last_error_message(void) { return tl_msg.c_str(); }
int alice_codec_device_count(void) {
    widen_hw_queues_once();
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}
int alice_codec_set_device(int device) {
    clear_error();
    int n = alice_codec_device_count();
    if (device < 0 || device >= n) return fail(kDeviceError, "device index out of range");
    tl_device = device;
    return ensure_device();
}
void alice_codec_trim(void) { pool().trim(); }
void alice_codec_test_force_first_cap(uint64_t cap) { tl_test_first_cap = cap; }

FrameEncoder* alice_codec_encoder_create_ex(uint8_t quality, uint8_t wavelet_type) {
    clear_error();
    if (wavelet_type > 2) { fail(kInvalidBitstream, "unknown wavelet type"); return nullptr; }
    return new (std::nothrow) FrameEncoder{quality, wavelet_type};
}
uint8_t alice_codec_encoder_quality(const FrameEncoder* e) { return e ? e->quality : 0; }
uint8_t alice_codec_encoder_wavelet(const FrameEncoder* e) { return e ? e->wavelet : 0; }
uint8_t alice_codec_chunk_wavelet(const EncodedChunk* c) { return c ? c->wavelet : 0; }
uint64_t alice_codec_chunk_compressed_size(const EncodedChunk* c) { return c ? c->data.size() : 0; }

AliceBatch* alice_codec_batch_create(uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks, uint8_t quality,
                                     uint8_t wavelet_type) {
    clear_error();
    if (wavelet_type > 2) { fail(kInvalidBitstream, "unknown wavelet type"); return nullptr; }
    ChunkDims d{};
    if (chunk_dims(width, height, frames, &d, n_chunks) || ensure_device()) return nullptr;
    tl_scope_stream = nullptr;   // the batch's buffers outlive every call: no stream of this thread's past belongs on them
    AliceBatch* b = new (std::nothrow) AliceBatch();
    if (!b) { fail(kOutOfMemory, "out of host memory"); return nullptr; }
    b->d = d; b->n_chunks = n_chunks; b->quality = quality; b->wavelet = wavelet_type; b->device = tl_device;
    // one ring of band slots serves the encode and the decode side (i16 both ways for every quality the bound covers)
    if (encode_work_alloc(b->enc, d, (int)n_chunks, inverse_scratch_bytes(d, true)) != kOk || b->evs.init() != kOk) { delete b; return nullptr; }
    return b;
}
void alice_codec_batch_destroy(AliceBatch* b) {
    if (!b) return;
    {
        // the caller's streams may be gone by now; drain the device the batch lives on before its buffers return to the pool
        DeviceScope ds(b->device);
        if (ds.ok) (void)hipDeviceSynchronize();
        b->enc_stream = b->dec_stream = nullptr;
        tl_scope_stream = nullptr;
    }
    delete b;
}

int alice_codec_batch_encode(AliceBatch* b, const void* d_rgb, void* hip_stream) {
    clear_error();
    if (!b || !d_rgb) return fail(kNullArgument, "null argument");
    std::vector<RgbLayout> rgb(b->n_chunks);
    for (uint32_t i = 0; i < b->n_chunks; ++i) rgb[i] = packed_rgb((const uint8_t*)d_rgb + (size_t)i * b->d.n_pixels * 3, b->d);
    return batch_encode_layouts(b, std::move(rgb), (hipStream_t)hip_stream);
}
int alice_codec_batch_encode_regions(AliceBatch* b, const void* d_frames, uint32_t frame_width, uint32_t frame_height,
                                     const uint32_t* origins, void* hip_stream) {
    clear_error();
    std::vector<RgbLayout> rgb;
    TRY(region_layouts(b, d_frames, frame_width, frame_height, origins, rgb));
    return batch_encode_layouts(b, std::move(rgb), (hipStream_t)hip_stream);
}
int alice_codec_batch_encode_finish(AliceBatch* b, uint64_t* sizes) {
    clear_error();
    if (!b) return fail(kNullArgument, "null argument");
    DeviceScope ds(b->device);
    if (!ds.ok) return tl_err;
    tl_scope_stream = nullptr;
    std::vector<RansResult> res;
    int rc = encode_collect(b->enc, b->enc_stream, res);
    // a chain outgrew its region: the capacities came from an earlier encode of other content (kCapReuse) -- size them
    // from this content's histograms and run again; should even that fall short (never observed), take the format's bound
    if (rc == kOverflowed && !b->last_rgb.empty())
        rc = encode_with_retry(b->last_rgb.data(), b->enc, b->quality, b->wavelet, b->enc_stream, &b->evs, kCapEstimate, nullptr, res,
                               b->chunk_qualities());
    if (rc == kOverflowed) return fail(kInternal, "rANS output exceeded the worst-case capacity");   // (no encode to repeat)
    if (rc) return rc;
    for (int i = 0; i < 4; ++i) (void)hipEventElapsedTime(&b->stage_ms[i], b->evs.ev[i], b->evs.ev[i + 1]);
    b->enc_timed = true;
    if (sizes)
        for (uint32_t i = 0; i < b->n_chunks; ++i)
            sizes[i] = (uint64_t)kAlcHeaderBytes + res[3 * i].len + res[3 * i + 1].len + res[3 * i + 2].len;
    return kOk;
}
int alice_codec_batch_predict_sizes(AliceBatch* b, const void* d_rgb, uint64_t* lo, uint64_t* hi, uint8_t* status, void* hip_stream) {
    clear_error();
    if (!b || !d_rgb || !lo || !hi || !status) return fail(kNullArgument, "null argument");
    DeviceScope ds(b->device);
    if (!ds.ok) return tl_err;
    tl_scope_stream = nullptr;
    std::vector<RgbLayout> rgb(b->n_chunks);
    for (uint32_t i = 0; i < b->n_chunks; ++i) rgb[i] = packed_rgb((const uint8_t*)d_rgb + (size_t)i * b->d.n_pixels * 3, b->d);
    std::vector<RateChannel> rc;
    TRY(predict_chunks(rgb.data(), b->n_chunks, b->d, b->wavelet, b->enc, (hipStream_t)hip_stream, nullptr, rc));
    for (uint32_t i = 0; i < b->n_chunks; ++i)
        rate_by_quality(rc.data() + (size_t)i * 192, lo + (size_t)i * kQualities, hi + (size_t)i * kQualities, status + (size_t)i * kQualities);
    return kOk;
}
int alice_codec_batch_set_qualities(AliceBatch* b, const uint8_t* qualities) {
    clear_error();
    if (!b) return fail(kNullArgument, "null argument");
    if (qualities) b->qualities.assign(qualities, qualities + b->n_chunks);
    else b->qualities.clear();
    return kOk;
}
int alice_codec_batch_encode_to_budget(AliceBatch* b, const void* d_rgb, const uint64_t* budgets, uint8_t min_q, uint8_t max_q,
                                       uint8_t* chosen, uint8_t* fits, void* hip_stream) {
    clear_error();
    if (!b || !d_rgb || !budgets || !chosen || !fits) return fail(kNullArgument, "null argument");
    TRY(check_quality_range(min_q, max_q));
    std::vector<uint64_t> lo((size_t)b->n_chunks * kQualities), hi(lo.size());
    std::vector<uint8_t> status(lo.size());
    TRY(alice_codec_batch_predict_sizes(b, d_rgb, lo.data(), hi.data(), status.data(), hip_stream));
    std::vector<uint8_t> q(b->n_chunks);
    for (uint32_t i = 0; i < b->n_chunks; ++i)
        q[i] = chosen[i] = choose_quality(hi.data() + (size_t)i * kQualities, status.data() + (size_t)i * kQualities, budgets[i],
                                          min_q, max_q, fits + i);
    TRY(alice_codec_batch_set_qualities(b, q.data()));
    return alice_codec_batch_encode(b, d_rgb, hip_stream);
}
const void* alice_codec_batch_alc_ptr(const AliceBatch* b, uint32_t chunk) {
    if (!b || chunk >= b->n_chunks) return nullptr;
    return b->enc.alc.as<uint8_t>() + (size_t)chunk * b->enc.alc_stride;
}
uint64_t alice_codec_batch_alc_stride(const AliceBatch* b) { return b ? b->enc.alc_stride : 0; }
const void* alice_codec_batch_symbols_ptr(const AliceBatch* b) { return b ? b->enc.sym.p : nullptr; }
// device memory the batch holds per chunk (symbols = decoded pixels, the .alc buffer at its current capacities, tables,
// histograms, results of both directions) and independent of the chunk count (transform scratch, the spare pixel buffer
// of a banded in-place decode): what a caller needs to size a batch to the free HBM
uint64_t alice_codec_batch_bytes_per_chunk(const AliceBatch* b) {
    if (!b) return 0;
    const uint64_t tables = 3ull * (sizeof(RansTable) + 256 * sizeof(uint32_t) + sizeof(RansResult));
    return 3 * b->d.padded + b->enc.alc_stride + 2 * tables + 3 * sizeof(RansDecodeDesc) + sizeof(unsigned long long);
}
uint64_t alice_codec_batch_fixed_bytes(const AliceBatch* b) {
    if (!b) return 0;
    uint64_t n = (uint64_t)b->enc.scratch.n + (16u << 20);   // + allocation granules of the small buffers
    if (transform_tiles_eligible(b->d) && inverse_cuts_chunk(b->d)) n += b->d.n_pixels * 3;
    return n;
}
uint64_t alice_codec_batch_padded_pixels(const AliceBatch* b) { return b ? b->d.padded : 0; }

int alice_codec_batch_pack_alc(AliceBatch* b, const uint64_t* sizes, void* d_dst, uint64_t dst_capacity, void* hip_stream) {
    clear_error();
    if (!b || !sizes || !d_dst) return fail(kNullArgument, "null argument");
    DeviceScope ds(b->device);
    if (!ds.ok) return tl_err;
    uint64_t off = 0;
    for (uint32_t i = 0; i < b->n_chunks; ++i) {
        if (sizes[i] > b->enc.alc_stride || off + sizes[i] > dst_capacity) return fail(kInvalidBufferSize, "pack buffer too small");
        HIP_TRY(hipMemcpyAsync((uint8_t*)d_dst + off, b->enc.alc.as<uint8_t>() + (size_t)i * b->enc.alc_stride, sizes[i],
                               hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
        off += sizes[i];
    }
    return kOk;
}

int alice_codec_batch_decode(AliceBatch* b, const void* d_alc, uint64_t alc_stride, void* d_rgb_out, void* hip_stream) {
    clear_error();
    if (!b || !d_alc) return fail(kNullArgument, "null argument");
    std::vector<RgbLayout> rgb;
    if (d_rgb_out) {
        rgb.resize(b->n_chunks);
        for (uint32_t i = 0; i < b->n_chunks; ++i) rgb[i] = packed_rgb((uint8_t*)d_rgb_out + (size_t)i * b->d.n_pixels * 3, b->d);
    }
    return batch_decode_layouts(b, d_alc, alc_stride, std::move(rgb), (hipStream_t)hip_stream);
}
int alice_codec_batch_decode_regions(AliceBatch* b, const void* d_alc, uint64_t alc_stride, void* d_frames_out, uint32_t frame_width,
                                     uint32_t frame_height, const uint32_t* origins, void* hip_stream) {
    clear_error();
    if (!d_alc) return fail(kNullArgument, "null argument");
    std::vector<RgbLayout> rgb;
    TRY(region_layouts(b, d_frames_out, frame_width, frame_height, origins, rgb));
    return batch_decode_layouts(b, d_alc, alc_stride, std::move(rgb), (hipStream_t)hip_stream);
}
const void* alice_codec_batch_rgb_ptr(const AliceBatch* b, uint32_t chunk) {
    if (!b || chunk >= b->n_chunks || chunk >= b->rgb_dst.size()) return nullptr;
    return b->rgb_dst[chunk].base;
}
int alice_codec_batch_decode_finish(AliceBatch* b) {
    clear_error();
    if (!b) return fail(kNullArgument, "null argument");
    DeviceScope ds(b->device);
    if (!ds.ok) return tl_err;
    TRY(decode_collect(b->dec, b->dec_stream));
    (void)hipEventElapsedTime(&b->stage_ms[4], b->evs.ev[5], b->evs.ev[6]);
    (void)hipEventElapsedTime(&b->stage_ms[5], b->evs.ev[6], b->evs.ev[7]);
    b->dec_timed = true;
    return kOk;
}
int alice_codec_batch_stage_ms(const AliceBatch* b, float out[6]) {
    if (!b || !out) return kNullArgument;
    for (int i = 0; i < 6; ++i) out[i] = b->stage_ms[i];
    return kOk;
}

// ---- stage level ----

int alice_codec_wavelet2d_forward(uint8_t k, int32_t* img, uint64_t w, uint64_t h) { clear_error(); return wavelet_nd(k, img, w, h, 1, 2, false); }
int alice_codec_wavelet2d_inverse(uint8_t k, int32_t* img, uint64_t w, uint64_t h) { clear_error(); return wavelet_nd(k, img, w, h, 1, 2, true); }
int alice_codec_wavelet3d_forward(uint8_t k, int32_t* v, uint64_t w, uint64_t h, uint64_t d) { clear_error(); return wavelet_nd(k, v, w, h, d, 3, false); }
int alice_codec_wavelet3d_inverse(uint8_t k, int32_t* v, uint64_t w, uint64_t h, uint64_t d) { clear_error(); return wavelet_nd(k, v, w, h, d, 3, true); }

int alice_codec_quantize_buffer(int32_t step, int32_t dead_zone, const int32_t* in, uint64_t n_in, int32_t* out, uint64_t n_out) {
    clear_error();
    if ((!in || !out) && n_in) return fail(kNullArgument, "null argument");
    if (n_out < n_in) return fail(kInvalidBufferSize, "buffer size mismatch: expected " + std::to_string(n_in) + ", got " + std::to_string(n_out));
    if (step == 0) return fail(kInvalidQuantStep, "step 0: the reference divides by zero");
    if (!n_in) return kOk;
    return staged<int32_t, int32_t>(in, n_in, out, n_in, [&](const int32_t* a, int32_t* b, hipStream_t st) { launch_quantize(a, b, n_in, step, dead_zone, st); });
}
int alice_codec_dequantize_buffer(int32_t step, const int32_t* in, uint64_t n_in, int32_t* out, uint64_t n_out) {
    clear_error();
    if ((!in || !out) && n_in) return fail(kNullArgument, "null argument");
    if (n_out < n_in) return fail(kInvalidBufferSize, "buffer size mismatch: expected " + std::to_string(n_in) + ", got " + std::to_string(n_out));
    if (!n_in) return kOk;
    return staged<int32_t, int32_t>(in, n_in, out, n_in, [&](const int32_t* a, int32_t* b, hipStream_t st) { launch_dequantize(a, b, n_in, step, st); });
}

FastQuantizer* alice_codec_fastquant_new(int32_t step) {
    clear_error();
    if (step <= 0) { fail(kInvalidQuantStep, "quantization step must be positive, got " + std::to_string(step)); return nullptr; }
    // src/quant.rs:200-216
    const uint32_t step_u = (uint32_t)step;
    const uint32_t extra = 32u - (uint32_t)__builtin_clz(step_u);
    const uint32_t shift = 32u + extra;
    const unsigned __int128 power = (unsigned __int128)1 << shift;
    const uint64_t rec = (uint64_t)((power + step_u - 1) / step_u);
    return new (std::nothrow) FastQuantizer{rec, shift, step, step};
}
FastQuantizer* alice_codec_fastquant_with_dead_zone(int32_t step, int32_t dead_zone) {
    FastQuantizer* q = alice_codec_fastquant_new(step);
    if (q) q->dead_zone = dead_zone;
    return q;
}
void alice_codec_fastquant_destroy(FastQuantizer* q) { delete q; }
int32_t alice_codec_fastquant_step(const FastQuantizer* q) { return q ? q->step : 0; }
int32_t alice_codec_fastquant_dead_zone(const FastQuantizer* q) { return q ? q->dead_zone : 0; }
int alice_codec_fastquant_quantize_buffer(const FastQuantizer* q, const int32_t* in, uint64_t n_in, int32_t* out, uint64_t n_out) {
    clear_error();
    if (!q || ((!in || !out) && n_in)) return fail(kNullArgument, "null argument");
    if (n_out < n_in) return fail(kInvalidBufferSize, "buffer size mismatch: expected " + std::to_string(n_in) + ", got " + std::to_string(n_out));
    if (!n_in) return kOk;
    return staged<int32_t, int32_t>(in, n_in, out, n_in, [&](const int32_t* a, int32_t* b, hipStream_t st) {
        launch_fast_quantize(a, b, n_in, q->reciprocal, q->shift, q->dead_zone, st);
    });
}
int alice_codec_fastquant_dequantize_buffer(const FastQuantizer* q, const int32_t* in, uint64_t n_in, int32_t* out, uint64_t n_out) {
    if (!q) { clear_error(); return fail(kNullArgument, "null argument"); }
    return alice_codec_dequantize_buffer(q->step, in, n_in, out, n_out);
}

int alice_codec_to_symbols(const int32_t* coeffs, uint64_t n, uint8_t* symbols, uint64_t n_out) {
    clear_error();
    if ((!coeffs || !symbols) && n) return fail(kNullArgument, "null argument");
    if (n_out < n) return fail(kInvalidBufferSize, "buffer size mismatch: expected " + std::to_string(n) + ", got " + std::to_string(n_out));
    if (!n) return kOk;
    return staged<int32_t, uint8_t>(coeffs, n, symbols, n, [&](const int32_t* a, uint8_t* b, hipStream_t st) { launch_to_symbols(a, b, n, st); });
}
int alice_codec_from_symbols(const uint8_t* symbols, uint64_t n, int32_t* coeffs, uint64_t n_out) {
    clear_error();
    if ((!coeffs || !symbols) && n) return fail(kNullArgument, "null argument");
    if (n_out < n) return fail(kInvalidBufferSize, "buffer size mismatch: expected " + std::to_string(n) + ", got " + std::to_string(n_out));
    if (!n) return kOk;
    return staged<uint8_t, int32_t>(symbols, n, coeffs, n, [&](const uint8_t* a, int32_t* b, hipStream_t st) { launch_from_symbols(a, b, n, st); });
}
int alice_codec_build_histogram(const uint8_t* symbols, uint64_t n, uint32_t hist[256]) {
    clear_error();
    if (!hist || (!symbols && n)) return fail(kNullArgument, "null argument");
    return staged<uint8_t, uint32_t>(symbols, n, hist, 256, [&](const uint8_t* a, uint32_t* b, hipStream_t st) {
        (void)hipMemsetAsync(b, 0, 256 * sizeof(uint32_t), st);
        launch_histogram(a, n, b, st);
    });
}

int alice_codec_freq_table_from_histogram(const uint32_t hist[256], uint16_t cum_freq[256], uint16_t freq[256]) {
    return alice_codec_freq_table_from_histogram_n(hist, 256, cum_freq, freq);
}
// FrequencyTable::from_histogram(&[u32]) for a slice of any length the u8 symbol API can address (src/rans.rs:102-150;
// the reference's own test_uniform_table_small uses 2, :934-944).  Entries from n_symbols on come back as (0, 0).
int alice_codec_freq_table_from_histogram_n(const uint32_t* hist, uint32_t n_symbols, uint16_t cum_freq[256], uint16_t freq[256]) {
    clear_error();
    if (!hist || !cum_freq || !freq) return fail(kNullArgument, "null argument");
    if (n_symbols == 0) return fail(kReferenceDiverges, "empty histogram: the reference divides by zero (uniform(0), src/rans.rs:159)");
    if (n_symbols > 256) return fail(kInvalidDimensions, "more than 256 symbols: the coders address symbols as u8");
    hipStream_t st;
    TRY(get_stream(&st));
    DevBuf h, t;
    TRY(h.alloc(256 * 4));
    TRY(t.alloc(sizeof(RansTable)));
    HIP_TRY(hipMemsetAsync(h.p, 0, 256 * 4, st));
    HIP_TRY(hipMemcpyAsync(h.p, hist, (size_t)n_symbols * 4, hipMemcpyHostToDevice, st));
    launch_rans_table(h.as<uint32_t>(), t.as<RansTable>(), 1, st, n_symbols);
    std::vector<RansTable> host(1);
    HIP_TRY(hipMemcpyAsync(host.data(), t.p, sizeof(RansTable), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < 256; ++i) { cum_freq[i] = (uint16_t)host[0].enc[i].cum; freq[i] = (uint16_t)host[0].enc[i].freq; }
    return kOk;
}

uint8_t* alice_codec_rans_encode(const uint8_t* symbols, uint64_t n, const uint16_t cum_freq[256], const uint16_t freq[256],
                                 uint64_t* out_len) {
    clear_error();
    if ((!symbols && n) || !cum_freq || !freq || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    uint8_t* p = nullptr;
    RansResult res{};
    if (stage_encode_chain(symbols, n, cum_freq, freq, kRansL, 0u, res, [&](uint64_t len) { return p = (uint8_t*)malloc(len ? len : 1); }) != kOk) {
        free(p);
        return nullptr;
    }
    *out_len = res.len;
    return p;
}

int alice_codec_rans_decode(const uint8_t* bytes, uint64_t len, const uint16_t cum_freq[256], const uint16_t freq[256],
                            uint64_t n, uint8_t* symbols) {
    clear_error();
    if ((!bytes && len) || !cum_freq || !freq || (!symbols && n)) return fail(kNullArgument, "null argument");
    if (!n) return kOk;
    hipStream_t st;
    TRY(get_stream(&st));
    DevBuf din;
    TRY(din.alloc(len + 16));
    if (len) HIP_TRY(hipMemcpyAsync(din.p, bytes, len, hipMemcpyHostToDevice, st));
    RansResult res{};
    return stage_decode_chain(st, din.as<uint8_t>(), len, cum_freq, freq, n, 0u, 0u, 0, symbols, res);
}
void alice_codec_test_last_decode_stats(uint32_t out[4]) { if (out) for (int i = 0; i < 4; ++i) out[i] = tl_dec_stats[i]; }

// ---- RansEncoder / RansDecoder as objects that live across calls (src/rans.rs:238-309, 321-389) ----

AliceRansEncoder* alice_codec_rans_encoder_new(void) { clear_error(); return new (std::nothrow) AliceRansEncoder(); }
void alice_codec_rans_encoder_destroy(AliceRansEncoder* e) { delete e; }
uint32_t alice_codec_rans_encoder_state(const AliceRansEncoder* e) { return e ? e->state : 0u; }

// encode_symbols(&mut self, symbols, table), :288-294: the symbols in reverse order, from the object's current state.
// Two calls s1 then s2 leave the same stream as one call on s2 || s1.
int alice_codec_rans_encoder_encode_symbols(AliceRansEncoder* e, const uint8_t* symbols, uint64_t n, const uint16_t cum_freq[256],
                                            const uint16_t freq[256]) {
    clear_error();
    if (!e || (!symbols && n) || !cum_freq || !freq) return fail(kNullArgument, "null argument");
    if (!n) return kOk;
    RansResult res{};
    std::vector<uint8_t> seg;
    TRY(stage_encode_chain(symbols, n, cum_freq, freq, e->state, 1u, res, [&](uint64_t len) { seg.resize((size_t)len); return seg.data(); }));
    e->state = res.final_state;
    e->bytes += res.len;
    e->segments.push_back(std::move(seg));
    return kOk;
}
// encode(&mut self, &RansSymbol), :269-285: one symbol given by its (cum_freq, freq) pair
int alice_codec_rans_encoder_encode(AliceRansEncoder* e, uint16_t cum_freq, uint16_t freq) {
    if (!e) { clear_error(); return fail(kNullArgument, "null argument"); }
    uint16_t c[256] = {0}, f[256] = {0};
    c[0] = cum_freq; f[0] = freq;
    const uint8_t sym = 0;
    return alice_codec_rans_encoder_encode_symbols(e, &sym, 1, c, f);
}
// finish(self), :298-308: consumes the encoder
uint8_t* alice_codec_rans_encoder_finish(AliceRansEncoder* e, uint64_t* out_len) {
    clear_error();
    if (!e || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    const uint64_t total = e->bytes + 4;
    uint8_t* p = (uint8_t*)malloc(total);
    if (!p) { fail(kOutOfMemory, "out of host memory"); return nullptr; }
    p[0] = (uint8_t)(e->state >> 24); p[1] = (uint8_t)(e->state >> 16); p[2] = (uint8_t)(e->state >> 8); p[3] = (uint8_t)e->state;
    uint64_t off = 4;
    for (size_t i = e->segments.size(); i-- > 0;) {
        if (!e->segments[i].empty()) memcpy(p + off, e->segments[i].data(), e->segments[i].size());
        off += e->segments[i].size();
    }
    *out_len = total;
    delete e;
    return p;
}

AliceRansDecoder* alice_codec_rans_decoder_new(const uint8_t* data, uint64_t len) {   // RansDecoder::new, :330-347
    clear_error();
    if (!data && len) { fail(kNullArgument, "null argument"); return nullptr; }
    AliceRansDecoder* d = new (std::nothrow) AliceRansDecoder();
    if (!d) { fail(kOutOfMemory, "out of host memory"); return nullptr; }
    d->input.assign(data, data + len);
    if (len >= 4) { d->state = ((uint32_t)data[0] << 24) | ((uint32_t)data[1] << 16) | ((uint32_t)data[2] << 8) | data[3]; d->pos = 4; }
    return d;
}
void alice_codec_rans_decoder_destroy(AliceRansDecoder* d) { delete d; }
int alice_codec_rans_decoder_is_empty(const AliceRansDecoder* d) {   // :385-389
    return d ? (d->pos >= d->input.size() && d->state < kRansL) : 1;
}
uint32_t alice_codec_rans_decoder_state(const AliceRansDecoder* d) { return d ? d->state : 0u; }
uint64_t alice_codec_rans_decoder_position(const AliceRansDecoder* d) { return d ? d->pos : 0u; }
// decode_n(&mut self, n, table), :375-381: the next n symbols, continuing from the current state and position
int alice_codec_rans_decoder_decode_n(AliceRansDecoder* d, uint64_t n, const uint16_t cum_freq[256], const uint16_t freq[256],
                                      uint8_t* symbols) {
    clear_error();
    if (!d || !cum_freq || !freq || (!symbols && n)) return fail(kNullArgument, "null argument");
    if (!n) return kOk;
    hipStream_t st;
    TRY(get_stream(&st));
    const uint64_t len = d->input.size();
    if (d->d_input.p && d->device != tl_device) d->d_input.reset();   // the calling thread moved to another device
    if (!d->d_input.p) {
        hipStream_t keep = tl_scope_stream;
        tl_scope_stream = nullptr;   // the copy outlives this call
        const int rc = d->d_input.alloc(len + 16);
        tl_scope_stream = keep;
        TRY(rc);
        d->device = tl_device;
        if (len) HIP_TRY(hipMemcpyAsync(d->d_input.p, d->input.data(), len, hipMemcpyHostToDevice, st));
    }
    RansResult res{};
    TRY(stage_decode_chain(st, d->d_input.as<uint8_t>(), len, cum_freq, freq, n, 1u, d->state, d->pos, symbols, res));
    d->state = res.final_state;
    d->pos = res.len;
    d->started = true;
    return kOk;
}

// quantize_subband / dequantize_subband (src/quant.rs:518-545): a sub-band's coefficients through a Quantizer
int alice_codec_quantize_subband(int32_t step, int32_t dead_zone, const int32_t* coeffs, uint64_t n, int32_t* out, uint64_t n_out) {
    return alice_codec_quantize_buffer(step, dead_zone, coeffs, n, out, n_out);
}
int alice_codec_dequantize_subband(int32_t step, const int32_t* coeffs, uint64_t n, int32_t* out, uint64_t n_out) {
    return alice_codec_dequantize_buffer(step, coeffs, n, out, n_out);
}

// ssim / ms_ssim (src/ssim.rs:63-176).  Returns the value, or -1.0 with the thread's error set (the Result::Err cases).
static int ssim_device(const uint8_t* d_a, const uint8_t* d_b, uint64_t w, uint64_t h, double* d_blocks, double* d_acc,
                       hipStream_t st, double* out) {
    const uint64_t bw = w / 8, bh = h / 8, nb = bw * bh;
    if (nb == 0) { *out = 1.0; return kOk; }                              // block_count == 0, :111-113
    launch_ssim_blocks(d_a, d_b, w, bw, nb, d_blocks, st);
    launch_ordered_sum_f64(d_blocks, nb, d_acc, st);
    double total = 0.0;
    HIP_TRY(hipMemcpyAsync(&total, d_acc, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out = total / (double)nb;
    return kOk;
}
static int ssim_impl(const uint8_t* a, uint64_t a_len, const uint8_t* b, uint64_t b_len, uint64_t w, uint64_t h, bool multi, double* out) {
    if (a_len != b_len) return fail(kInvalidBufferSize, "buffer size mismatch: expected " + std::to_string(a_len) + ", got " + std::to_string(b_len));
    unsigned __int128 wh = (unsigned __int128)w * h;
    if (wh != a_len) return fail(kInvalidBufferSize, "buffer size mismatch: expected " + std::to_string((uint64_t)wh) + ", got " + std::to_string(a_len));
    if (a_len == 0) { *out = 1.0; return kOk; }
    if (!a || !b) return fail(kNullArgument, "null argument");
    hipStream_t st;
    TRY(get_stream(&st));
    DevBuf da, db, da2, db2, dblk, dacc;
    TRY(da.alloc(a_len)); TRY(db.alloc(a_len)); TRY(dblk.alloc(((w / 8) * (h / 8) + 1) * sizeof(double))); TRY(dacc.alloc(8));
    HIP_TRY(hipMemcpyAsync(da.p, a, a_len, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(db.p, b, a_len, hipMemcpyHostToDevice, st));
    if (!multi) return ssim_device(da.as<uint8_t>(), db.as<uint8_t>(), w, h, dblk.as<double>(), dacc.as<double>(), st, out);
    TRY(da2.alloc(a_len / 4 + 1)); TRY(db2.alloc(a_len / 4 + 1));
    const double weights[3] = {0.3333, 0.3333, 0.3334};
    uint8_t *ca = da.as<uint8_t>(), *cb = db.as<uint8_t>(), *na = da2.as<uint8_t>(), *nb = db2.as<uint8_t>();
    uint64_t cw = w, ch = h;
    double result = 0.0;
    for (int wi = 0; wi < 3; ++wi) {
        const double weight = weights[wi];
        double s = 0.0;
        TRY(ssim_device(ca, cb, cw, ch, dblk.as<double>(), dacc.as<double>(), st, &s));
        double l = log(s > 0.0 ? s : 0.0);                                   // s.max(0.0).ln().max(-10.0), :146
        if (!(l > -10.0)) l = -10.0;
        result += weight * l;
        const uint64_t nw = cw / 2, nh = ch / 2;
        if (nw < 8 || nh < 8) {
            // the reference finds the current weight by value (first match), :153-163: the second scale maps to
            // index 0 again and counts weights[1] once more
            int pos = 0;
            for (int k = 0; k < 3; ++k) if (fabs(weights[k] - weight) < 1e-10) { pos = k; break; }
            for (int k = pos + 1; k < 3; ++k) result += weights[k] * l;
            break;
        }
        launch_downsample2(ca, cw, ch, na, st);
        launch_downsample2(cb, cw, ch, nb, st);
        std::swap(ca, na); std::swap(cb, nb);
        cw = nw; ch = nh;
    }
    *out = exp(result);
    return kOk;
}
double alice_codec_ssim(const uint8_t* a, uint64_t a_len, const uint8_t* b, uint64_t b_len, uint64_t width, uint64_t height) {
    clear_error();
    double v = -1.0;
    return ssim_impl(a, a_len, b, b_len, width, height, false, &v) == kOk ? v : -1.0;
}
double alice_codec_ms_ssim(const uint8_t* a, uint64_t a_len, const uint8_t* b, uint64_t b_len, uint64_t width, uint64_t height) {
    clear_error();
    double v = -1.0;
    return ssim_impl(a, a_len, b, b_len, width, height, true, &v) == kOk ? v : -1.0;
}

// AnalyticalRDO (src/quant.rs:377-505) + SubBand3D::quant_strength (src/lib.rs:149-158)
double alice_codec_rdo_target_bpp(uint8_t quality) {   // with_quality, :398-411
    const double RCP_100 = 1.0 / 100.0;
    const unsigned qq = quality > 100 ? 100u : quality;
    const double q = (double)qq * RCP_100;
    return fma(q * q, 23.9, 0.1);
}
uint8_t alice_codec_subband_quant_strength(uint8_t subband) {
    switch (subband) { case 0: return 1; case 1: case 2: case 4: return 2; case 3: case 5: case 6: return 4; default: return 8; }
}
int alice_codec_rdo_compute_quantizer(double target_bpp, const int32_t* coeffs, uint64_t n, uint8_t subband, int32_t* step,
                                      int32_t* dead_zone) {
    clear_error();
    if ((!coeffs && n) || !step || !dead_zone) return fail(kNullArgument, "null argument");
    if (subband > 7) return fail(kInvalidDimensions, "unknown sub-band");
    double variance = 1.0;                                           // estimate_variance of an empty slice, :415-417
    if (n) {
        hipStream_t st;
        TRY(get_stream(&st));
        DevBuf dx, dsum, dacc;
        TRY(dx.alloc(n * sizeof(int32_t))); TRY(dsum.alloc(8)); TRY(dacc.alloc(8));
        HIP_TRY(hipMemcpyAsync(dx.p, coeffs, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(dsum.p, 0, 8, st));
        launch_sum_i32(dx.as<int32_t>(), n, dsum.as<unsigned long long>(), st);
        long long sum = 0;
        HIP_TRY(hipMemcpyAsync(&sum, dsum.p, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const double inv_n = 1.0 / (double)n;
        const double mean = (double)sum * inv_n;                      // :421-424
        launch_ordered_sqdev_sum(dx.as<int32_t>(), n, mean, dacc.as<double>(), st);
        double acc = 0.0;
        HIP_TRY(hipMemcpyAsync(&acc, dacc.p, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        variance = acc * inv_n;                                       // :426-433
        if (!(variance > 1.0)) variance = 1.0;                        // f64::max(1.0)
    }
    const double lambda = (6.0 * M_LN2 * variance) / target_bpp;      // :440-443
    const double r = round(sqrt(12.0 * lambda));                      // :448-451
    int32_t base = r != r ? 0 : (r >= 2147483647.0 ? INT32_MAX : (r <= -2147483648.0 ? INT32_MIN : (int32_t)r));
    if (base < 1) base = 1;
    int32_t s = (int32_t)((uint32_t)base * (uint32_t)alice_codec_subband_quant_strength(subband));   // :461-462
    if (s < 1) s = 1;
    *step = s;
    *dead_zone = (int32_t)((uint32_t)s + (uint32_t)(s / 2));          // :465
    return kOk;
}

// InterleavedRansEncoder::{encode, finish} (src/rans.rs:393-456): four independent single-stream coders over the
// sub-sequences i = j mod 4, behind a 32-byte header (4 stream lengths, 4 symbol counts, u32 LE).  On the GPU
// that is four chains of the same encode kernel running side by side.
static int rans_encode_interleaved_impl(const uint8_t* symbols, uint64_t n, const uint16_t cum_freq[256], const uint16_t freq[256],
                                        uint8_t** out, uint64_t* out_len) {
    if ((!symbols && n) || !cum_freq || !freq || !out_len) return fail(kNullArgument, "null argument");
    hipStream_t st;
    TRY(get_stream(&st));
    uint64_t cnt[4];
    for (int j = 0; j < 4; ++j) cnt[j] = (n + 3 - j) / 4;        // :423-425
    if (cnt[0] > 0xFFFFFFFFull) return fail(kDimensionOverflow, "symbol count does not fit the u32 header field");
    const uint64_t stride = round_up(cnt[0] + 16, 256);
    const uint64_t cap = round_up(2 * cnt[0] + 4 + 64 + 64, 256);
    DevBuf ds, d4, dt, dout, dres;
    RansTable* tables = nullptr;
    TRY(ds.alloc(n)); TRY(d4.alloc(4 * stride)); TRY(dout.alloc(4 * cap)); TRY(dres.alloc(4 * sizeof(RansResult)));
    if (n) HIP_TRY(hipMemcpyAsync(ds.p, symbols, n, hipMemcpyHostToDevice, st));
    launch_split4(ds.as<uint8_t>(), n, d4.as<uint8_t>(), stride, st);
    TRY(stage_tables(cum_freq, freq, 4, dt, st, &tables));
    std::vector<RansEncodeDesc> enc(4);
    for (int j = 0; j < 4; ++j)
        enc[j] = RansEncodeDesc{d4.as<uint8_t>() + (size_t)j * stride, cnt[j], tables + j, dout.as<uint8_t>() + (size_t)j * cap, cap,
                                dres.as<RansResult>() + j, kRansL, 0u};
    TRY(hub_chains(st, std::move(enc), {}, cnt[0]));
    RansResult res[4];
    HIP_TRY(hipMemcpyAsync(res, dres.p, sizeof(res), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t total = 32;
    for (int j = 0; j < 4; ++j) {
        TRY(encode_flags_error(res[j].flags));
        if (res[j].flags & kRansOverflow) return fail(kInternal, "rANS output exceeded the worst-case capacity");
        if (res[j].len > 0xFFFFFFFFull) return fail(kDimensionOverflow, "stream length does not fit the u32 header field");
        total += res[j].len;
    }
    uint8_t* p = *out = (uint8_t*)malloc(total);   // (the caller frees it on failure)
    if (!p) return fail(kOutOfMemory, "out of host memory");
    uint64_t off = 32;
    for (int j = 0; j < 4; ++j) {
        const uint32_t l = (uint32_t)res[j].len, c = (uint32_t)cnt[j];
        memcpy(p + 4 * j, &l, 4);
        memcpy(p + 16 + 4 * j, &c, 4);
        HIP_TRY(hipMemcpyAsync(p + off, dout.as<uint8_t>() + (size_t)j * cap + (cap - res[j].len), res[j].len, hipMemcpyDeviceToHost, st));
        off += res[j].len;
    }
    HIP_TRY(hipStreamSynchronize(st));
    *out_len = total;
    return kOk;
}
uint8_t* alice_codec_rans_encode_interleaved(const uint8_t* symbols, uint64_t n, const uint16_t cum_freq[256],
                                             const uint16_t freq[256], uint64_t* out_len) {
    clear_error();
    uint8_t* p = nullptr;
    if (rans_encode_interleaved_impl(symbols, n, cum_freq, freq, &p, out_len) == kOk) return p;
    free(p);
    return nullptr;
}

// InterleavedRansDecoder::{new, decode_n} (src/rans.rs:468-519; SimdRansDecoder reads the same format): the four
// streams are decoded by four chains, then merged in the reference's round-robin order (streams that run out
// are skipped).  Where the reference would index out of bounds or spin forever this returns an error.
int alice_codec_rans_decode_interleaved(const uint8_t* bytes, uint64_t len, const uint16_t cum_freq[256],
                                        const uint16_t freq[256], uint64_t n, uint8_t* symbols) {
    clear_error();
    if ((!bytes && len) || !cum_freq || !freq || (!symbols && n)) return fail(kNullArgument, "null argument");
    if (len < 32) return fail(kInvalidBitstream, "interleaved stream shorter than its 32-byte header");
    uint64_t slen[4], cnt[4], total = 0, end = 32;
    for (int j = 0; j < 4; ++j) {
        uint32_t a, b;
        memcpy(&a, bytes + 4 * j, 4); memcpy(&b, bytes + 16 + 4 * j, 4);
        slen[j] = a; cnt[j] = b; total += b; end += a;
    }
    if (end > len) return fail(kInvalidBitstream, "stream lengths exceed the input");
    if (n > total) return fail(kReferenceDiverges, "more symbols requested than the header counts hold: the reference decoder does not terminate");
    if (!n) return kOk;
    // symbols of stream j that land below position n: pos(j, k) = sum_i min(cnt_i, k) + #{i < j : cnt_i > k}
    auto pos = [&](int j, uint64_t k) {
        uint64_t p = 0;
        for (int i = 0; i < 4; ++i) { p += std::min(cnt[i], k); if (i < j && cnt[i] > k) ++p; }
        return p;
    };
    uint64_t need[4], mx = 0;
    for (int j = 0; j < 4; ++j) {
        uint64_t lo = 0, hi = cnt[j];      // first k with pos(j, k) >= n
        while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (pos(j, mid) >= n) hi = mid; else lo = mid + 1; }
        need[j] = lo; mx = std::max(mx, lo);
    }
    hipStream_t st;
    TRY(get_stream(&st));
    const uint64_t stride = round_up(mx + 16, 256);
    DevBuf din, dt, d4, dout, dres;
    RansTable* table = nullptr;
    TRY(din.alloc(len + 16)); TRY(d4.alloc(4 * stride)); TRY(dout.alloc(n)); TRY(dres.alloc(4 * sizeof(RansResult)));
    HIP_TRY(hipMemcpyAsync(din.p, bytes, len, hipMemcpyHostToDevice, st));
    TRY(stage_tables(cum_freq, freq, 1, dt, st, &table));
    std::vector<RansDecodeDesc> desc(4);
    uint64_t off = 32;
    for (int j = 0; j < 4; ++j) {
        desc[j] = RansDecodeDesc{din.as<uint8_t>() + off, slen[j], d4.as<uint8_t>() + (size_t)j * stride, need[j], table, 0u, 0u, 0, dres.as<RansResult>() + j};
        off += slen[j];
    }
    TRY(hub_chains(st, {}, std::move(desc), mx));
    launch_merge4(d4.as<uint8_t>(), stride, need, cnt, dout.as<uint8_t>(), n, st);
    RansResult res[4];
    HIP_TRY(hipMemcpyAsync(res, dres.p, sizeof(res), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(symbols, dout.p, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (auto& r : res)
        if (r.flags & kRansInternal) return fail(kInternal, "decode table outside the packed range (freq > 4096 with live slots)");
    return kOk;
}

int alice_codec_rgb_to_ycocg_r(const uint8_t* rgb, uint64_t rgb_len, int16_t* y, int16_t* co, int16_t* cg, uint64_t n_out) {
    clear_error();
    if (rgb_len % 3 != 0) return fail(kInvalidBufferSize, "rgb length is not a multiple of 3");  // src/color.rs:205-210
    const uint64_t n = rgb_len / 3;
    if (n_out < n) return fail(kInvalidBufferSize, "output planes too small");                   // :212-218
    if (!n) return kOk;
    if (!rgb || !y || !co || !cg) return fail(kNullArgument, "null argument");
    hipStream_t st;
    TRY(get_stream(&st));
    DevBuf a, b;
    TRY(a.alloc(rgb_len)); TRY(b.alloc(3 * n * 2));
    HIP_TRY(hipMemcpyAsync(a.p, rgb, rgb_len, hipMemcpyHostToDevice, st));
    int16_t* p = b.as<int16_t>();
    launch_rgb_to_ycocg(a.as<uint8_t>(), n, p, p + n, p + 2 * n, st);
    HIP_TRY(hipMemcpyAsync(y, p, n * 2, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(co, p + n, n * 2, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(cg, p + 2 * n, n * 2, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}
int alice_codec_ycocg_r_to_rgb(const int16_t* y, const int16_t* co, const int16_t* cg, uint64_t n, uint8_t* rgb, uint64_t rgb_len) {
    clear_error();
    if (rgb_len < n * 3) return fail(kInvalidBufferSize, "rgb buffer too small");  // src/color.rs:258-263
    if (!n) return kOk;
    if (!rgb || !y || !co || !cg) return fail(kNullArgument, "null argument");
    hipStream_t st;
    TRY(get_stream(&st));
    DevBuf a, b;
    TRY(a.alloc(3 * n * 2)); TRY(b.alloc(n * 3));
    int16_t* p = a.as<int16_t>();
    HIP_TRY(hipMemcpyAsync(p, y, n * 2, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(p + n, co, n * 2, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(p + 2 * n, cg, n * 2, hipMemcpyHostToDevice, st));
    launch_ycocg_to_rgb(p, p + n, p + 2 * n, n, b.as<uint8_t>(), st);
    HIP_TRY(hipMemcpyAsync(rgb, b.p, n * 3, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}

// ---- many chunks from host memory in one call: the chunk driver's fast path (the chains of all chunks run side
// by side; a single chunk is bound by its three serial chains) ----

static int validate_decode_many(const EncodedChunk* const* chunks, uint32_t n_chunks, uint8_t* rgb_out, uint64_t rgb_out_len, ChunkDims* d) {
    if (!chunks || (!rgb_out && rgb_out_len)) return fail(kNullArgument, "null argument");
    if (n_chunks == 0) return kOk;
    for (uint32_t i = 0; i < n_chunks; ++i) {
        if (!chunks[i]) return fail(kNullArgument, "null chunk");
        if (chunks[i]->width != chunks[0]->width || chunks[i]->height != chunks[0]->height || chunks[i]->frames != chunks[0]->frames)
            return fail(kInvalidDimensions, "chunks of one call must have the same shape");
    }
    for (uint32_t i = 0; i < n_chunks; ++i) TRY(validate_for_decode(*chunks[i], d, chunks[i]->data.size()));
    if (d->n_pixels == 0) return rgb_out_len == 0 ? kOk : fail(kInvalidBufferSize, "output buffer size mismatch");
    if (rgb_out_len != d->n_pixels * 3 * n_chunks)
        return fail(kInvalidBufferSize, "buffer size mismatch: expected " + std::to_string(d->n_pixels * 3 * n_chunks) + ", got " + std::to_string(rgb_out_len));
    return kOk;
}

int alice_codec_encode_many(const FrameEncoder* encoder, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                            uint32_t frames, uint32_t n_chunks, EncodedChunk** out_chunks) {
    clear_error();
    ChunkDims d{};
    TRY(validate_encode_many(encoder, rgb, rgb_len, width, height, frames, n_chunks, out_chunks, &d));
    return encode_chunks_on_device(*encoder, rgb, d, out_chunks, n_chunks);
}

int alice_codec_decode_many(const EncodedChunk* const* chunks, uint32_t n_chunks, uint8_t* rgb_out, uint64_t rgb_out_len) {
    clear_error();
    ChunkDims d{};
    TRY(validate_decode_many(chunks, n_chunks, rgb_out, rgb_out_len, &d));
    return decode_chunks_on_device(chunks, d, rgb_out, n_chunks);
}

// ---- the same over several GPUs of the node: chunk k goes to devices[k mod n_devices] (64-frame chunks are independent
// bitstreams, src/pipeline.rs:461-497: no cross-chunk state), one host thread per listed device, every
// device moves its own chunks over its own PCIe link, results land in the caller's arrays in chunk order ----

int alice_codec_many_devices_plan(uint32_t n_chunks, const int* devices, uint32_t n_devices, int* device_of_chunk) {
    clear_error();
    if ((!devices && n_devices) || (!device_of_chunk && n_chunks)) return fail(kNullArgument, "null argument");
    if (n_devices == 0) return fail(kDeviceError, "empty device list");
    for (uint32_t i = 0; i < n_devices; ++i)
        if (devices[i] < 0) return fail(kDeviceError, "negative device index");
    for (uint32_t k = 0; k < n_chunks; ++k) device_of_chunk[k] = devices[k % n_devices];
    return kOk;
}

}  // extern "C"
namespace {
// runs fn(slot) on one thread per slot of the device list, each bound to its device; returns the first failure
template <typename Fn>
int run_on_devices(const int* devices, uint32_t n_devices, Fn fn) {
    const int count = alice_codec_device_count();
    for (uint32_t i = 0; i < n_devices; ++i)
        if (devices[i] >= count) return fail(kDeviceError, "device index " + std::to_string(devices[i]) + " out of range (" + std::to_string(count) + " visible)");
    return on_threads(n_devices, [&](uint32_t s) { return devices[s]; }, [&](uint32_t s) {
        int rc = ensure_device();
        if (rc == kOk) rc = fn(s);
        return rc == kOk ? rc : fail(rc, "device " + std::to_string(devices[s]) + ": " + tl_msg);
    });
}
}  // namespace
extern "C" {

int alice_codec_encode_many_devices(const FrameEncoder* encoder, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                                    uint32_t frames, uint32_t n_chunks, const int* devices, uint32_t n_devices, EncodedChunk** out_chunks) {
    clear_error();
    ChunkDims d{};
    TRY(validate_encode_many(encoder, rgb, rgb_len, width, height, frames, n_chunks, out_chunks, &d));
    std::vector<int> plan(n_chunks);
    TRY(alice_codec_many_devices_plan(n_chunks, devices, n_devices, plan.data()));
    if (n_chunks == 0) return kOk;
    const int rc = run_on_devices(devices, n_devices, [&](uint32_t slot) {
        return encode_chunks_on_device(*encoder, rgb, d, out_chunks, n_chunks, slot, n_devices);
    });
    if (rc != kOk)
        for (uint32_t k = 0; k < n_chunks; ++k) { delete out_chunks[k]; out_chunks[k] = nullptr; }
    return rc;
}

int alice_codec_decode_many_devices(const EncodedChunk* const* chunks, uint32_t n_chunks, const int* devices, uint32_t n_devices,
                                    uint8_t* rgb_out, uint64_t rgb_out_len) {
    clear_error();
    ChunkDims d{};
    TRY(validate_decode_many(chunks, n_chunks, rgb_out, rgb_out_len, &d));
    std::vector<int> plan(n_chunks);
    TRY(alice_codec_many_devices_plan(n_chunks, devices, n_devices, plan.data()));
    if (n_chunks == 0 || d.n_pixels == 0) return kOk;
    return run_on_devices(devices, n_devices, [&](uint32_t slot) {
        return decode_chunks_on_device(chunks, d, rgb_out, n_chunks, slot, n_devices);
    });
}

// ---- PART 2: rate control ----

int alice_codec_predict_sizes(uint8_t wavelet_type, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                              uint32_t frames, uint64_t lo[101], uint64_t hi[101], uint8_t status[101]) {
    clear_error();
    if (!lo || !hi || !status || (!rgb && rgb_len)) return fail(kNullArgument, "null argument");
    if (wavelet_type > 2) return fail(kInvalidBitstream, "unknown wavelet type");
    return predict_sizes_host(wavelet_type, rgb, rgb_len, width, height, frames, lo, hi, status);
}

EncodedChunk* alice_codec_encode_to_size(uint8_t wavelet_type, const uint8_t* rgb, uint64_t rgb_len, uint32_t width,
                                         uint32_t height, uint32_t frames, uint64_t max_bytes, uint8_t min_q, uint8_t max_q,
                                         uint8_t* chosen_q, uint8_t* fits) {
    clear_error();
    if (!chosen_q || !fits || (!rgb && rgb_len)) { fail(kNullArgument, "null argument"); return nullptr; }
    if (wavelet_type > 2) { fail(kInvalidBitstream, "unknown wavelet type"); return nullptr; }
    EncodedChunk* c = nullptr;
    return encode_to_size_host(wavelet_type, rgb, rgb_len, width, height, frames, max_bytes, min_q, max_q, chosen_q, fits, &c) == kOk ? c : nullptr;
}

int alice_codec_dev_predict_sizes(const void* d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                  uint8_t wavelet_type, uint64_t* lo, uint64_t* hi, uint8_t* status, void* d_step_hist,
                                  void* hip_stream) {
    clear_error();
    if (!d_rgb || !lo || !hi || !status) return fail(kNullArgument, "null argument");
    if (wavelet_type > 2) return fail(kInvalidBitstream, "unknown wavelet type");
    ChunkDims d{};
    TRY(chunk_dims(width, height, frames, &d, n_chunks));
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);   // temporaries drain the caller's stream before they return to the pool
    EncodeWork w;
    w.d = d; w.n_chunks = 1;
    if (transform_tiles_eligible(d)) TRY(w.scratch.alloc(forward_scratch_bytes(d)));
    std::vector<RgbLayout> layouts(n_chunks);
    for (uint32_t i = 0; i < n_chunks; ++i) layouts[i] = packed_rgb((const uint8_t*)d_rgb + (size_t)i * d.n_pixels * 3, d);
    std::vector<RateChannel> rc;
    TRY(predict_chunks(layouts.data(), n_chunks, d, wavelet_type, w, st, (uint32_t*)d_step_hist, rc));
    for (uint32_t i = 0; i < n_chunks; ++i)
        rate_by_quality(rc.data() + (size_t)i * 192, lo + (size_t)i * kQualities, hi + (size_t)i * kQualities, status + (size_t)i * kQualities);
    return kOk;
}

// ---- PART 3: device-resident stage calls (building blocks of the row-slab sharded path) ----
// Every pointer named d_* is a device pointer; launches go on `hip_stream` and the call returns after the
// stream has drained (the rANS calls need their result on the host anyway).

static int dev_forward_symbols(const void* d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint8_t wavelet_type,
                               uint8_t quality, void* d_symbols, void* d_hist, void* hip_stream, bool wide) {
    clear_error();
    if (!d_rgb || !d_symbols) return fail(kNullArgument, "null argument");
    if (wavelet_type > 2) return fail(kInvalidBitstream, "unknown wavelet type");
    ChunkDims d{};
    TRY(chunk_dims(width, height, frames, &d));
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);   // temporaries drain the caller's stream before they return to the pool
    EncodeWork w;
    w.d = d; w.n_chunks = 1;
    if (transform_tiles_eligible(d)) TRY(w.scratch.alloc(forward_scratch_bytes(d)));
    TRY(w.hist.alloc(3 * 256 * sizeof(uint32_t)));
    uint32_t* hist = d_hist ? (uint32_t*)d_hist : w.hist.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(hist, 0, 3 * 256 * sizeof(uint32_t), st));
    TRY(forward_chunk(packed_rgb(d_rgb, d), d, wavelet_type, quality_to_step(quality), w, (uint8_t*)d_symbols, hist, st, wide));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}

int alice_codec_dev_forward_symbols(const void* d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint8_t wavelet_type,
                                    uint8_t quality, void* d_symbols, void* d_hist, void* hip_stream) {
    return dev_forward_symbols(d_rgb, width, height, frames, wavelet_type, quality, d_symbols, d_hist, hip_stream, false);
}

int alice_codec_dev_forward_symbols_wide(const void* d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint8_t wavelet_type,
                                         uint8_t quality, void* d_symbols, void* d_hist, void* hip_stream) {
    return dev_forward_symbols(d_rgb, width, height, frames, wavelet_type, quality, d_symbols, d_hist, hip_stream, true);
}

int alice_codec_dev_inverse_symbols(const void* d_symbols, uint32_t width, uint32_t height, uint32_t frames, uint8_t wavelet_type,
                                    const int32_t step[3], void* d_rgb, void* hip_stream) {
    clear_error();
    if (!d_rgb || !d_symbols || !step) return fail(kNullArgument, "null argument");
    if (wavelet_type > 2) return fail(kInvalidBitstream, "unknown wavelet type");
    ChunkDims d{};
    TRY(chunk_dims(width, height, frames, &d));
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);   // temporaries drain the caller's stream before they return to the pool
    DecodeWork w;
    w.d = d; w.n_chunks = 1;
    if (transform_tiles_eligible(d)) TRY(w.scratch_own.alloc(inverse_scratch_bytes(d, inverse_bounds(wavelet_type, step).mid16)));
    TRY(inverse_chunk((const uint8_t*)d_symbols, d, wavelet_type, step, w.scratch_own.p, w, packed_rgb(d_rgb, d), st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}

static int dev_wavelet3d(uint8_t k, void* d_volume, void* d_tmp, uint64_t w, uint64_t h, uint64_t d, bool inverse, void* hip_stream) {
    clear_error();
    if (!d_volume || !d_tmp) return fail(kNullArgument, "null argument");
    if (k > 2) return fail(kInvalidBitstream, "unknown wavelet type");
    unsigned __int128 tot = (unsigned __int128)w * h * d;
    if (tot > ((unsigned __int128)1 << 40)) return fail(kDimensionOverflow, "volume too large");
    if (tot == 0) return kOk;
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    wavelet_on_device(k, (int32_t*)d_volume, (int32_t*)d_tmp, w, h, d, 3, inverse, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}
int alice_codec_dev_wavelet3d_forward(uint8_t k, void* d_volume, void* d_tmp, uint64_t w, uint64_t h, uint64_t d, void* hip_stream) {
    return dev_wavelet3d(k, d_volume, d_tmp, w, h, d, false, hip_stream);
}
int alice_codec_dev_wavelet3d_inverse(uint8_t k, void* d_volume, void* d_tmp, uint64_t w, uint64_t h, uint64_t d, void* hip_stream) {
    return dev_wavelet3d(k, d_volume, d_tmp, w, h, d, true, hip_stream);
}

int alice_codec_dev_histogram(const void* d_symbols, uint64_t n, void* d_hist, void* hip_stream) {
    clear_error();
    if (!d_hist || (!d_symbols && n)) return fail(kNullArgument, "null argument");
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);   // temporaries drain the caller's stream before they return to the pool
    HIP_TRY(hipMemsetAsync(d_hist, 0, 256 * sizeof(uint32_t), st));
    if (n) launch_histogram((const uint8_t*)d_symbols, n, (uint32_t*)d_hist, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}

uint64_t alice_codec_rans_stream_bound(const uint32_t hist[256], uint64_t n) {
    if (!hist) return round_up(2 * n + 4 + 64 + 64, 256);
    const uint64_t worst = round_up(2 * n + 4 + 64 + 64, 256);
    const uint64_t est = round_up(estimate_stream_cap(hist, n) + 64, 256);
    return est < worst ? est : worst;
}

int alice_codec_dev_rans_encode(const void* d_symbols, uint64_t n, const uint32_t hist[256], void* d_out, uint64_t cap,
                                uint64_t* out_offset, uint64_t* out_len, void* hip_stream) {
    clear_error();
    if ((!d_symbols && n) || !hist || !d_out || !out_offset || !out_len) return fail(kNullArgument, "null argument");
    if (cap < 4 + 64 + 64) return fail(kInvalidBufferSize, "stream region too small");
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);   // temporaries drain the caller's stream before they return to the pool
    DevBuf dh, dt, dres;
    TRY(dh.alloc(2 * 256 * 4)); TRY(dt.alloc(sizeof(RansTable))); TRY(dres.alloc(sizeof(RansResult)));
    HIP_TRY(hipMemcpyAsync(dh.p, hist, 256 * 4, hipMemcpyHostToDevice, st));
    // `hist` is the caller's word: the table is built from it, but which of its entries the chain will meet is counted
    // from the symbols themselves (one pass, nothing next to a serial chain).  A table flagged clean on the strength of a
    // histogram that is not the data's would send a symbol of frequency 0 or above 4096 through the one-compare step.
    uint32_t* const d_used = dh.as<uint32_t>() + 256;
    HIP_TRY(hipMemsetAsync(d_used, 0, 256 * 4, st));
    if (n) launch_histogram((const uint8_t*)d_symbols, n, d_used, st);
    launch_rans_table(dh.as<uint32_t>(), dt.as<RansTable>(), 1, st, 256, d_used);
    launch_rans_encode((const uint8_t*)d_symbols, n, n, dt.as<RansTable>(), (uint8_t*)d_out, cap, dres.as<RansResult>(), 1, st);
    RansResult res{};
    HIP_TRY(hipMemcpyAsync(&res, dres.p, sizeof(res), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    TRY(encode_flags_error(res.flags));
    if (res.flags & kRansOverflow) return fail(kInvalidBufferSize, "stream region too small for this chain (use alice_codec_rans_stream_bound(NULL, n))");
    *out_len = res.len;
    *out_offset = cap - res.len;
    return kOk;
}

int alice_codec_dev_rans_decode(const void* d_stream, uint64_t len, const uint32_t hist[256], void* d_symbols, uint64_t n,
                                void* hip_stream) {
    clear_error();
    if ((!d_stream && len) || !hist || (!d_symbols && n)) return fail(kNullArgument, "null argument");
    if (!n) return kOk;
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);   // temporaries drain the caller's stream before they return to the pool
    DevBuf dh, dt, ddesc, dres;
    TRY(dh.alloc(256 * 4)); TRY(dt.alloc(sizeof(RansTable))); TRY(ddesc.alloc(sizeof(RansDecodeDesc))); TRY(dres.alloc(sizeof(RansResult)));
    HIP_TRY(hipMemcpyAsync(dh.p, hist, 256 * 4, hipMemcpyHostToDevice, st));
    RansDecodeDesc desc{(const uint8_t*)d_stream, len, (uint8_t*)d_symbols, n, dt.as<RansTable>()};
    HIP_TRY(hipMemcpyAsync(ddesc.p, &desc, sizeof(desc), hipMemcpyHostToDevice, st));
    launch_rans_table(dh.as<uint32_t>(), dt.as<RansTable>(), 1, st);
    launch_rans_decode(ddesc.as<RansDecodeDesc>(), dres.as<RansResult>(), 1, st);
    RansResult res{};
    HIP_TRY(hipMemcpyAsync(&res, dres.p, sizeof(res), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    note_decode_stats(res);
    if (res.flags & kRansInternal) return fail(kInternal, "rANS decode table invariant violated");
    return kOk;
}


// ---- test and measurement hooks (include/alice_codec_test.h) ----

void alice_codec_test_set_tuning(long band_kb) { set_transform_tuning(band_kb); }
void alice_codec_test_set_value_table_radius(int r) { set_value_table_radius(r); }
void alice_codec_test_set_grid_cap(uint32_t max_blocks) { set_generic_grid_cap(max_blocks); }
int alice_codec_test_wide_symbols(const int32_t* coeffs, uint64_t n, uint8_t* out) {
    clear_error();
    if (!coeffs || !out) return fail(kNullArgument, "null argument");
    return staged<int32_t, uint8_t>(coeffs, n, out, 1024 + 6 * n, [&](const int32_t* a, uint8_t* b, hipStream_t st) {
        uint32_t* hist = (uint32_t*)b;
        int32_t* back = (int32_t*)(b + 1024);
        uint16_t* z = (uint16_t*)(b + 1024 + 4 * n);
        (void)hipMemsetAsync(hist, 0, 1024, st);
        launch_to_symbols_wide(a, z, n, st);
        launch_from_symbols_wide(z, back, n, st);
        launch_histogram_wide(z, n, hist, st);
    });
}
void alice_codec_test_rate_log_table(uint32_t lo[4097], uint32_t hi[4097], uint32_t g[2]) {
    const RateLogTable& t = rate_log_table();
    if (lo) memcpy(lo, t.lo, sizeof(t.lo));
    if (hi) memcpy(hi, t.hi, sizeof(t.hi));
    if (g) { g[0] = t.g_up; g[1] = t.g_dn; }
}
int alice_codec_test_inverse_variant(uint8_t wavelet_type, const int32_t step[3], int wide) {
    if (wavelet_type > 2 || !step) return -1;
    const InverseBounds ib = inverse_bounds(wavelet_type, step, wide ? kWideMaxQ : kByteMaxQ);   // as inverse_chunk does
    return inverse_variant(ib.exact, ib.mid16, ib.lds16);
}
int alice_codec_test_set_admission_budget(uint64_t bytes) {
    clear_error();
    TRY(ensure_device());
    ChainHub::of_device(tl_device)->set_budget((size_t)bytes);
    return kOk;
}

// ns != nullptr: chain c decodes ns[c] symbols (alice_codec_test_decode_chains_n); else every chain decodes n
static int test_decode_chains(uint32_t n_chains, const void* const* d_streams, const uint64_t* lens, const uint16_t* cum_freq,
                              const uint16_t* freq, void* const* d_symbols, uint64_t n, const uint64_t* ns, uint32_t* out, void* hip_stream) {
    clear_error();
    if (!n_chains || !d_streams || !lens || !cum_freq || !freq || !d_symbols || !out || (!ns && !n)) return fail(kNullArgument, "null argument");
    for (uint32_t c = 0; ns && c < n_chains; ++c)
        if (!ns[c]) return fail(kNullArgument, "null argument");
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    DevBuf dt, ddesc, dres;
    TRY(dt.alloc((size_t)n_chains * (1024 + sizeof(RansTable))));   // every chain's (cum, freq) arrays, then the tables
    TRY(ddesc.alloc((size_t)n_chains * sizeof(RansDecodeDesc)));
    TRY(dres.alloc((size_t)n_chains * sizeof(RansResult)));
    uint16_t* const arrays = dt.as<uint16_t>();
    RansTable* const tables = (RansTable*)(dt.as<uint8_t>() + (size_t)n_chains * 1024);
    HIP_TRY(hipMemcpy2DAsync(arrays, 1024, cum_freq, 512, 512, n_chains, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpy2DAsync(arrays + 256, 1024, freq, 512, 512, n_chains, hipMemcpyHostToDevice, st));
    std::vector<RansDecodeDesc> descs(n_chains);
    for (uint32_t c = 0; c < n_chains; ++c) {
        launch_rans_table_from_arrays(arrays + 512 * (size_t)c, arrays + 512 * (size_t)c + 256, tables + c, st);
        descs[c] = RansDecodeDesc{(const uint8_t*)d_streams[c], lens[c], (uint8_t*)d_symbols[c], ns ? ns[c] : n, tables + c, 0u, 0u, 0ull, nullptr};
    }
    HIP_TRY(hipMemcpyAsync(ddesc.p, descs.data(), descs.size() * sizeof(RansDecodeDesc), hipMemcpyHostToDevice, st));
    launch_rans_decode(ddesc.as<RansDecodeDesc>(), dres.as<RansResult>(), (int)n_chains, st);
    std::vector<RansResult> res(n_chains);
    HIP_TRY(hipMemcpyAsync(res.data(), dres.p, res.size() * sizeof(RansResult), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t c = 0; c < n_chains; ++c) {
        out[4 * c] = (uint32_t)(res[c].len > 0xFFFFFFFFull ? 0xFFFFFFFFull : res[c].len);
        out[4 * c + 1] = res[c].final_state;
        out[4 * c + 2] = res[c].paths;
        out[4 * c + 3] = res[c].fast_tiles;
        if (res[c].flags & kRansInternal) return fail(kInternal, "rANS decode kernel invariant violated");
    }
    return kOk;
}
int alice_codec_test_decode_chains(uint32_t n_chains, const void* const* d_streams, const uint64_t* lens, const uint16_t* cum_freq,
                                   const uint16_t* freq, void* const* d_symbols, uint64_t n, uint32_t* out, void* hip_stream) {
    return test_decode_chains(n_chains, d_streams, lens, cum_freq, freq, d_symbols, n, nullptr, out, hip_stream);
}
int alice_codec_test_decode_chains_n(uint32_t n_chains, const void* const* d_streams, const uint64_t* lens, const uint16_t* cum_freq,
                                     const uint16_t* freq, void* const* d_symbols, const uint64_t* ns, uint32_t* out, void* hip_stream) {
    if (!ns) return fail(kNullArgument, "null argument");
    return test_decode_chains(n_chains, d_streams, lens, cum_freq, freq, d_symbols, 0ull, ns, out, hip_stream);
}

int alice_codec_test_decode_chains_ex(uint32_t n_chains, const void* const* d_streams, const uint64_t* lens, void* const* d_symbols,
                                      const uint64_t* ns, const uint32_t* hists, const uint16_t* cum_freq, const uint16_t* freq,
                                      const uint32_t* from_arrays, const uint32_t* resume, const uint32_t* x0, const uint64_t* pos0,
                                      const uint32_t* own_result, uint32_t* out, void* hip_stream) {
    clear_error();
    const bool arrays_given = cum_freq && freq;
    if (!n_chains || !d_streams || !lens || !d_symbols || !ns || !out || (!hists && !arrays_given) || (from_arrays && (!hists || !arrays_given)) ||
        (resume && (!x0 || !pos0)))
        return fail(kNullArgument, "null argument");
    for (uint32_t c = 0; c < n_chains; ++c)
        if ((!d_streams[c] && lens[c]) || (!d_symbols[c] && ns[c])) return fail(kNullArgument, "null argument");
    // no decoder object stands behind the end of its stream, and the kernel's window arithmetic relies on it
    for (uint32_t c = 0; resume && c < n_chains; ++c)
        if (resume[c] && pos0[c] > lens[c]) return fail(kInvalidBufferSize, "resume position behind the end of the stream");
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    // per kind of table: every chain's histogram or (cum, freq) arrays, then the tables
    DevBuf dth, dta, ddesc, dres;
    RansTable *tables_h = nullptr, *tables_a = nullptr;
    if (hists) {
        TRY(dth.alloc((size_t)n_chains * (1024 + sizeof(RansTable))));
        tables_h = (RansTable*)(dth.as<uint8_t>() + (size_t)n_chains * 1024);
        HIP_TRY(hipMemcpyAsync(dth.p, hists, (size_t)n_chains * 1024, hipMemcpyHostToDevice, st));
        launch_rans_table(dth.as<uint32_t>(), tables_h, (int)n_chains, st);
    }
    if (arrays_given) {
        TRY(dta.alloc((size_t)n_chains * (1024 + sizeof(RansTable))));
        tables_a = (RansTable*)(dta.as<uint8_t>() + (size_t)n_chains * 1024);
        uint16_t* const d_cum = dta.as<uint16_t>();
        uint16_t* const d_freq = d_cum + (size_t)n_chains * 256;
        HIP_TRY(hipMemcpyAsync(d_cum, cum_freq, (size_t)n_chains * 512, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_freq, freq, (size_t)n_chains * 512, hipMemcpyHostToDevice, st));
        launch_rans_tables_from_arrays(d_cum, d_freq, tables_a, (int)n_chains, st);
    }
    // results[c] of the launch, then a RansResult of its own per chain; both filled with a pattern no chain writes, so that a
    // chain that reports into the wrong one (or into both) is seen
    TRY(ddesc.alloc((size_t)n_chains * sizeof(RansDecodeDesc)));
    TRY(dres.alloc(2 * (size_t)n_chains * sizeof(RansResult)));
    HIP_TRY(hipMemsetAsync(dres.p, 0xA5, 2 * (size_t)n_chains * sizeof(RansResult), st));
    RansResult* const shared = dres.as<RansResult>();
    RansResult* const own = shared + n_chains;
    std::vector<RansDecodeDesc> descs(n_chains);
    for (uint32_t c = 0; c < n_chains; ++c) {
        const bool arr = from_arrays ? from_arrays[c] != 0u : !hists;
        const bool res = resume && resume[c];
        descs[c] = RansDecodeDesc{(const uint8_t*)d_streams[c], lens[c], (uint8_t*)d_symbols[c], ns[c], (arr ? tables_a : tables_h) + c,
                                  res ? 1u : 0u, res ? x0[c] : 0u, res ? pos0[c] : 0ull, own_result && own_result[c] ? own + c : nullptr};
    }
    HIP_TRY(hipMemcpyAsync(ddesc.p, descs.data(), descs.size() * sizeof(RansDecodeDesc), hipMemcpyHostToDevice, st));
    launch_rans_decode(ddesc.as<RansDecodeDesc>(), shared, (int)n_chains, st);
    HIP_TRY(hipGetLastError());
    std::vector<RansResult> res(2 * (size_t)n_chains);
    HIP_TRY(hipMemcpyAsync(res.data(), dres.p, res.size() * sizeof(RansResult), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    bool internal = false, misplaced = false;
    for (uint32_t c = 0; c < n_chains; ++c) {
        const bool mine = own_result && own_result[c];
        const RansResult& r = res[(mine ? n_chains : 0u) + c];
        const uint8_t* const other = (const uint8_t*)&res[(mine ? 0u : n_chains) + c];
        for (size_t b = 0; b < sizeof(RansResult); ++b) misplaced |= other[b] != 0xA5u;
        uint32_t* const o = out + 6 * (size_t)c;
        o[0] = (uint32_t)(r.len > 0xFFFFFFFFull ? 0xFFFFFFFFull : r.len);
        o[1] = r.final_state;
        o[2] = r.paths;
        o[3] = r.fast_tiles;
        o[4] = r.slow_tiles;
        o[5] = r.flags;
        internal |= (r.flags & kRansInternal) != 0u;
    }
    if (misplaced) return fail(kInternal, "a decode chain wrote a RansResult that is not its own");
    if (internal) return fail(kInternal, "rANS decode kernel invariant violated");
    return kOk;
}

// out_stride: 6 (alice_codec_test_encode_chains) or 7 (..._blocks: RansResult.comp_blocks behind the six)
static int test_encode_chains(uint32_t n_chains, const void* const* d_symbols, const uint64_t* ns, const uint32_t* hists,
                              const uint16_t* cum_freq, const uint16_t* freq, void* const* d_regions, const uint64_t* caps,
                              const uint32_t* x_init, const uint32_t* keep_open, uint32_t* out, uint32_t out_stride, void* hip_stream) {
    clear_error();
    if (!n_chains || !d_symbols || !ns || (!hists && (!cum_freq || !freq)) || !d_regions || !caps || !out) return fail(kNullArgument, "null argument");
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    DevBuf dt, ddesc, dres;
    TRY(dt.alloc((size_t)n_chains * (1024 + sizeof(RansTable))));   // every chain's histogram or (cum, freq) arrays, then the tables
    TRY(ddesc.alloc((size_t)n_chains * sizeof(RansEncodeDesc)));
    TRY(dres.alloc((size_t)n_chains * sizeof(RansResult)));
    RansTable* const tables = (RansTable*)(dt.as<uint8_t>() + (size_t)n_chains * 1024);
    if (hists) {
        HIP_TRY(hipMemcpyAsync(dt.p, hists, (size_t)n_chains * 1024, hipMemcpyHostToDevice, st));
        launch_rans_table(dt.as<uint32_t>(), tables, (int)n_chains, st);
    } else {
        uint16_t* const arrays = dt.as<uint16_t>();
        HIP_TRY(hipMemcpy2DAsync(arrays, 1024, cum_freq, 512, 512, n_chains, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpy2DAsync(arrays + 256, 1024, freq, 512, 512, n_chains, hipMemcpyHostToDevice, st));
        for (uint32_t c = 0; c < n_chains; ++c)
            launch_rans_table_from_arrays(arrays + 512 * (size_t)c, arrays + 512 * (size_t)c + 256, tables + c, st);
    }
    std::vector<RansEncodeDesc> descs(n_chains);
    for (uint32_t c = 0; c < n_chains; ++c) {
        if ((!d_symbols[c] && ns[c]) || !d_regions[c]) return fail(kNullArgument, "null argument");
        descs[c] = RansEncodeDesc{(const uint8_t*)d_symbols[c], ns[c], tables + c, (uint8_t*)d_regions[c], caps[c], dres.as<RansResult>() + c,
                                  x_init ? x_init[c] : kRansL, keep_open ? keep_open[c] : 0u};
    }
    HIP_TRY(hipMemcpyAsync(ddesc.p, descs.data(), descs.size() * sizeof(RansEncodeDesc), hipMemcpyHostToDevice, st));
    launch_rans_encode_descs(ddesc.as<RansEncodeDesc>(), (int)n_chains, st);
    HIP_TRY(hipGetLastError());
    std::vector<RansResult> res(n_chains);
    HIP_TRY(hipMemcpyAsync(res.data(), dres.p, res.size() * sizeof(RansResult), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t c = 0; c < n_chains; ++c) {
        uint32_t* const o = out + (size_t)out_stride * c;
        o[0] = (uint32_t)(res[c].len > 0xFFFFFFFFull ? 0xFFFFFFFFull : res[c].len);
        o[1] = res[c].final_state;
        o[2] = res[c].flags;
        o[3] = res[c].paths;
        o[4] = res[c].fast_tiles;
        o[5] = res[c].slow_tiles;
        if (out_stride > 6u) o[6] = res[c].comp_blocks;
    }
    return kOk;
}

int alice_codec_test_encode_chains(uint32_t n_chains, const void* const* d_symbols, const uint64_t* ns, const uint32_t* hists,
                                   const uint16_t* cum_freq, const uint16_t* freq, void* const* d_regions, const uint64_t* caps,
                                   const uint32_t* x_init, const uint32_t* keep_open, uint32_t* out, void* hip_stream) {
    return test_encode_chains(n_chains, d_symbols, ns, hists, cum_freq, freq, d_regions, caps, x_init, keep_open, out, 6u, hip_stream);
}

int alice_codec_test_encode_chains_blocks(uint32_t n_chains, const void* const* d_symbols, const uint64_t* ns, const uint32_t* hists,
                                          const uint16_t* cum_freq, const uint16_t* freq, void* const* d_regions,
                                          const uint64_t* caps, const uint32_t* x_init, const uint32_t* keep_open, uint32_t* out,
                                          void* hip_stream) {
    return test_encode_chains(n_chains, d_symbols, ns, hists, cum_freq, freq, d_regions, caps, x_init, keep_open, out, 7u, hip_stream);
}

int alice_codec_test_chain_occupancy(uint32_t out[6]) {
    clear_error();
    if (!out) return fail(kNullArgument, "null argument");
    TRY(ensure_device());
    if (!chain_kernel_occupancy(out)) return fail(kDeviceError, "hipFuncGetAttributes / occupancy query failed");
    return kOk;
}

int alice_codec_test_transform_ms(const void* d_rgb, void* d_sym, void* d_rgb_out, uint32_t n_buffers, uint32_t width,
                                  uint32_t height, uint32_t frames, uint8_t wavelet_type, uint8_t quality, uint32_t n_chunks,
                                  uint32_t reps, int probe, float out_ms[2], void* hip_stream) {
    clear_error();
    if (!d_rgb || !d_sym || !d_rgb_out || !out_ms || !n_buffers || !n_chunks || !reps) return fail(kNullArgument, "null argument");
    if (wavelet_type > 2) return fail(kInvalidBitstream, "unknown wavelet type");
    uint64_t n_pixels = 0;
    TRY(checked_pixel_count(width, height, frames, &n_pixels));
    if (n_pixels == 0) return fail(kInvalidDimensions, "invalid dimensions");
    const ChunkDims d = make_dims(width, height, frames);
    if (!transform_tiles_eligible(d)) return fail(kInvalidDimensions, "shape runs the generic path: nothing to time");
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    const int32_t step = quality_to_step(quality);
    const int32_t steps[3] = {step, step, step};
    const InverseBounds ib = inverse_bounds(wavelet_type, steps);
    DevBuf scratch, hist;
    TRY(scratch.alloc(std::max(forward_scratch_bytes(d), inverse_scratch_bytes(d, ib.mid16))));
    TRY(hist.alloc(3 * 256 * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(hist.p, 0, 3 * 256 * sizeof(uint32_t), st));
    StageEvents ev;
    TRY(ev.init());
    set_transform_probe(probe);
    auto fwd = [&]() {
        for (uint32_t c = 0; c < n_chunks; ++c) {
            const uint32_t k = c % n_buffers;
            launch_forward_transform(packed_rgb((const uint8_t*)d_rgb + (size_t)k * d.n_pixels * 3, d), d, wavelet_type, step, scratch.p,
                                     (uint8_t*)d_sym + (size_t)k * 3 * d.padded, hist.as<uint32_t>(), st);
        }
    };
    auto inv = [&]() {
        for (uint32_t c = 0; c < n_chunks; ++c) {
            const uint32_t k = c % n_buffers;
            launch_inverse_transform((const uint8_t*)d_sym + (size_t)k * 3 * d.padded, d, wavelet_type, steps, ib.exact, ib.mid16,
                                     ib.lds16, scratch.p, packed_rgb((uint8_t*)d_rgb_out + (size_t)k * d.n_pixels * 3, d), st);
        }
    };
    fwd();   // warm-up; also leaves real symbols for the inverse
    hipError_t e = hipEventRecord(ev.ev[0], st);
    for (uint32_t r = 0; r < reps && e == hipSuccess; ++r) fwd();
    if (e == hipSuccess) e = hipEventRecord(ev.ev[1], st);
    inv();
    if (e == hipSuccess) e = hipEventRecord(ev.ev[2], st);
    for (uint32_t r = 0; r < reps && e == hipSuccess; ++r) inv();
    if (e == hipSuccess) e = hipEventRecord(ev.ev[3], st);
    set_transform_probe(0);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(kDeviceError, hipGetErrorString(e));
    float a = 0.f, b = 0.f;
    HIP_TRY(hipEventElapsedTime(&a, ev.ev[0], ev.ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, ev.ev[2], ev.ev[3]));
    out_ms[0] = a / (float)(reps * n_chunks);
    out_ms[1] = b / (float)(reps * n_chunks);
    return kOk;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// segmentation (src/segment.rs; kernels in segment.hip)
// ------------------------------------------------------------------------------------------
namespace {

// width * height as the reference's u32 `total` (src/segment.rs:179, :242): a product past u32 wraps in a release build
// and panics in a debug one, here it is an error before any device work
int segment_total(uint32_t w, uint32_t h, uint64_t* total) {
    const uint64_t t = (uint64_t)w * h;
    if (t > 0xFFFFFFFFull) return fail(kDimensionOverflow, "width * height does not fit u32");
    *total = t;
    return kOk;
}

// extract_person_rgb indexes the mask with u32 arithmetic (src/segment.rs:111-113): every index of the bbox walk must fit
int bbox_indices_fit(uint32_t width, const uint32_t bbox[4]) {
    const uint64_t bx = bbox[0], by = bbox[1], bw = bbox[2], bh = bbox[3];
    if (by + bh > 0xFFFFFFFFull || bx + bw > 0xFFFFFFFFull) return fail(kDimensionOverflow, "bbox end does not fit u32");
    if (bw && bh && (by + bh - 1) * width + bx + bw - 1 > 0xFFFFFFFFull)
        return fail(kDimensionOverflow, "bbox index row * width + col does not fit u32");
    return kOk;
}

// one segmentation on device buffers; d_mask may be null; total > 0
int segment_on_device(const SegSource& src, uint32_t w, uint32_t h, uint32_t n_frames, uint32_t rd, uint32_t re, uint8_t* d_mask,
                      uint32_t* d_stats, hipStream_t st) {
    DevBuf scratch;
    const uint64_t sb = segment_scratch_bytes(w, h, n_frames, rd, re);
    if (sb) TRY(scratch.alloc(sb));
    launch_segment(src, w, h, n_frames, rd, re, scratch.p, d_mask, d_stats, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}

// host planes in, host mask / bbox / count out (the shared tail of segment_by_motion and segment_by_chroma)
int segment_host(SegSource src, const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes, uint32_t w, uint32_t h,
                 uint32_t rd, uint32_t re, uint8_t* mask, uint32_t bbox[4], uint32_t* count) {
    const uint64_t total = (uint64_t)w * h;
    TRY(ensure_device());
    hipStream_t st;
    TRY(get_stream(&st));
    DevBuf da, db, dm, ds;
    TRY(da.alloc(a_bytes));
    if (b) TRY(db.alloc(b_bytes));
    TRY(dm.alloc(total));
    TRY(ds.alloc(5 * sizeof(uint32_t)));
    HIP_TRY(hipMemcpyAsync(da.p, a, a_bytes, hipMemcpyHostToDevice, st));
    if (b) HIP_TRY(hipMemcpyAsync(db.p, b, b_bytes, hipMemcpyHostToDevice, st));
    if (src.kind == kSegMotion) { src.cur = da.as<uint8_t>(); src.ref = db.as<uint8_t>(); }
    else src.cg = da.as<int16_t>();
    TRY(segment_on_device(src, w, h, 1, rd, re, dm.as<uint8_t>(), ds.as<uint32_t>(), st));
    uint32_t stats[5];
    HIP_TRY(hipMemcpyAsync(mask, dm.p, total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(stats, ds.p, sizeof(stats), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(bbox, stats, 4 * sizeof(uint32_t));
    *count = stats[4];
    return kOk;
}

int empty_segment(uint32_t bbox[4], uint32_t* count) {
    bbox[0] = bbox[1] = bbox[2] = bbox[3] = 0;
    *count = 0;
    return kOk;
}

// RLE of n > 0 device bytes into d_out (>= 3n); *out_len = bytes written
int rle_on_device(const uint8_t* d_mask, uint64_t n, uint8_t* d_out, uint64_t* out_len, hipStream_t st) {
    DevBuf scratch, dn;
    TRY(scratch.alloc(rle_scratch_bytes(n)));
    TRY(dn.alloc(sizeof(unsigned long long)));
    launch_rle(d_mask, n, d_out, scratch.p, dn.as<unsigned long long>(), st);
    HIP_TRY(hipGetLastError());
    unsigned long long pieces = 0;
    HIP_TRY(hipMemcpyAsync(&pieces, dn.p, sizeof(pieces), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out_len = pieces * 3;
    return kOk;
}

int extract_on_device(const uint8_t* d_mask, uint64_t mask_len, const uint8_t* d_rgb, uint64_t rgb_len, uint32_t width,
                      const uint32_t bbox[4], uint8_t* d_out, uint64_t* out_len, hipStream_t st) {
    DevBuf scratch, dn;
    TRY(scratch.alloc(compact_scratch_bytes((uint64_t)bbox[2] * bbox[3])));
    TRY(dn.alloc(sizeof(unsigned long long)));
    launch_extract_person(d_mask, mask_len, d_rgb, rgb_len, width, bbox, d_out, scratch.p, dn.as<unsigned long long>(), st);
    HIP_TRY(hipGetLastError());
    unsigned long long px = 0;
    HIP_TRY(hipMemcpyAsync(&px, dn.p, sizeof(px), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out_len = px * 3;
    return kOk;
}

}  // namespace
extern "C" {

int alice_codec_segment_by_motion(const uint8_t* current, uint64_t current_len, const uint8_t* reference, uint64_t reference_len,
                                  uint32_t width, uint32_t height, uint8_t motion_threshold, uint32_t dilate_radius,
                                  uint32_t erode_radius, uint8_t* mask, uint64_t mask_len, uint32_t bbox[4],
                                  uint32_t* foreground_count) {
    clear_error();
    if (!bbox || !foreground_count || (!current && current_len) || (!reference && reference_len) || (!mask && mask_len))
        return fail(kNullArgument, "null argument");
    uint64_t total = 0;
    TRY(segment_total(width, height, &total));
    if (current_len < total)   // src/segment.rs:180-185
        return fail(kInvalidBufferSize, "buffer size mismatch: expected " + std::to_string(total) + ", got " + std::to_string(current_len));
    if (reference_len < total)   // :186-191
        return fail(kInvalidBufferSize, "buffer size mismatch: expected " + std::to_string(total) + ", got " + std::to_string(reference_len));
    if (mask_len < total) return fail(kInvalidBufferSize, "mask buffer too small: need " + std::to_string(total));
    if (!total) return empty_segment(bbox, foreground_count);
    SegSource src{};
    src.kind = kSegMotion; src.motion_threshold = motion_threshold;
    return segment_host(src, current, total, reference, total, width, height, dilate_radius, erode_radius, mask, bbox, foreground_count);
}

int alice_codec_segment_by_chroma(const int16_t* cg, uint64_t cg_len, uint32_t width, uint32_t height, int16_t green_threshold,
                                  uint8_t* mask, uint64_t mask_len, uint32_t bbox[4], uint32_t* foreground_count) {
    clear_error();
    if (!bbox || !foreground_count || (!cg && cg_len) || (!mask && mask_len)) return fail(kNullArgument, "null argument");
    uint64_t total = 0;
    TRY(segment_total(width, height, &total));
    // the reference indexes past a short cg and panics (src/segment.rs:245-253)
    if (cg_len < total)
        return fail(kInvalidBufferSize, "buffer size mismatch: expected " + std::to_string(total) + ", got " + std::to_string(cg_len));
    if (mask_len < total) return fail(kInvalidBufferSize, "mask buffer too small: need " + std::to_string(total));
    if (!total) return empty_segment(bbox, foreground_count);
    SegSource src{};
    src.kind = kSegCg; src.green_threshold = green_threshold;
    return segment_host(src, cg, total * sizeof(int16_t), nullptr, 0, width, height, 2, 1, mask, bbox, foreground_count);   // :253-254
}

uint64_t alice_codec_rle_bound(uint64_t n) { return n > UINT64_MAX / 3 ? UINT64_MAX : 3 * n; }

uint8_t* alice_codec_rle_encode_mask(const uint8_t* mask, uint64_t n, uint64_t* out_len) {
    clear_error();
    if (!out_len || (!mask && n)) { fail(kNullArgument, "null argument"); return nullptr; }
    if (n > UINT64_MAX / 3) { fail(kDimensionOverflow, "mask too long"); return nullptr; }
    if (!n) {   // an empty mask encodes to nothing (src/segment.rs:132-134)
        uint8_t* p = (uint8_t*)malloc(1);
        if (!p) { fail(kOutOfMemory, "out of host memory"); return nullptr; }
        *out_len = 0;
        return p;
    }
    if (ensure_device() != kOk) return nullptr;
    hipStream_t st;
    if (get_stream(&st) != kOk) return nullptr;
    DevBuf dm, dout;
    uint64_t len = 0;
    int rc = dm.alloc(n);
    if (rc == kOk) rc = dout.alloc(3 * n);
    if (rc == kOk && hipMemcpyAsync(dm.p, mask, n, hipMemcpyHostToDevice, st) != hipSuccess) rc = fail(kDeviceError, "copy failed");
    if (rc == kOk) rc = rle_on_device(dm.as<uint8_t>(), n, dout.as<uint8_t>(), &len, st);
    if (rc != kOk) return nullptr;
    uint8_t* p = (uint8_t*)malloc(len ? len : 1);
    if (!p) { fail(kOutOfMemory, "out of host memory"); return nullptr; }
    if (hipMemcpyAsync(p, dout.p, len, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        free(p);
        fail(kDeviceError, "copy failed");
        return nullptr;
    }
    *out_len = len;
    return p;
}

int alice_codec_extract_person_rgb(const uint8_t* mask, uint64_t mask_len, uint32_t width, const uint32_t bbox[4],
                                   const uint8_t* rgb, uint64_t rgb_len, uint8_t* out, uint64_t out_cap, uint64_t* out_len) {
    clear_error();
    if (!bbox || !out_len || (!mask && mask_len) || (!rgb && rgb_len) || (!out && out_cap)) return fail(kNullArgument, "null argument");
    TRY(bbox_indices_fit(width, bbox));
    const uint64_t items = (uint64_t)bbox[2] * bbox[3];
    if (out_cap < 3 * (unsigned __int128)items)
        return fail(kInvalidBufferSize, "output buffer too small: need 3 * bbox w * h = " + std::to_string(3 * (unsigned __int128)items > UINT64_MAX ? UINT64_MAX : 3 * items));
    *out_len = 0;
    if (!items || !mask_len || rgb_len < 3) return kOk;   // nothing passes the guards of src/segment.rs:114-116
    TRY(ensure_device());
    hipStream_t st;
    TRY(get_stream(&st));
    DevBuf dm, dr, dout;
    TRY(dm.alloc(mask_len));
    TRY(dr.alloc(rgb_len));
    TRY(dout.alloc(3 * items));
    HIP_TRY(hipMemcpyAsync(dm.p, mask, mask_len, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dr.p, rgb, rgb_len, hipMemcpyHostToDevice, st));
    uint64_t len = 0;
    TRY(extract_on_device(dm.as<uint8_t>(), mask_len, dr.as<uint8_t>(), rgb_len, width, bbox, dout.as<uint8_t>(), &len, st));
    HIP_TRY(hipMemcpyAsync(out, dout.p, len, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out_len = len;
    return kOk;
}

int alice_codec_dev_segment_motion(const void* d_current, const void* d_reference, uint64_t reference_stride, uint32_t width,
                                   uint32_t height, uint32_t n_frames, uint8_t motion_threshold, uint32_t dilate_radius,
                                   uint32_t erode_radius, void* d_mask, void* d_stats, void* hip_stream) {
    clear_error();
    if (!d_current || !d_reference || !d_stats) return fail(kNullArgument, "null argument");
    uint64_t total = 0;
    TRY(segment_total(width, height, &total));
    if (!n_frames) return kOk;
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);   // temporaries drain the caller's stream before they return to the pool
    if (!total) {
        HIP_TRY(hipMemsetAsync(d_stats, 0, (size_t)n_frames * 5 * sizeof(uint32_t), st));
        HIP_TRY(hipStreamSynchronize(st));
        return kOk;
    }
    SegSource src{};
    src.kind = kSegMotion; src.cur = (const uint8_t*)d_current; src.ref = (const uint8_t*)d_reference;
    src.ref_stride = reference_stride; src.motion_threshold = motion_threshold;
    return segment_on_device(src, width, height, n_frames, dilate_radius, erode_radius, (uint8_t*)d_mask, (uint32_t*)d_stats, st);
}

int alice_codec_dev_segment_chroma_rgb(const void* d_rgb, uint32_t width, uint32_t height, uint32_t n_frames, int16_t green_threshold,
                                       void* d_mask, void* d_stats, void* hip_stream) {
    clear_error();
    if (!d_rgb || !d_stats) return fail(kNullArgument, "null argument");
    uint64_t total = 0;
    TRY(segment_total(width, height, &total));
    if (!n_frames) return kOk;
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    if (!total) {
        HIP_TRY(hipMemsetAsync(d_stats, 0, (size_t)n_frames * 5 * sizeof(uint32_t), st));
        HIP_TRY(hipStreamSynchronize(st));
        return kOk;
    }
    SegSource src{};
    src.kind = kSegRgb; src.rgb = (const uint8_t*)d_rgb; src.green_threshold = green_threshold;
    return segment_on_device(src, width, height, n_frames, 2, 1, (uint8_t*)d_mask, (uint32_t*)d_stats, st);
}

int alice_codec_dev_rle_encode_mask(const void* d_mask, uint64_t n, void* d_out, uint64_t cap, uint64_t* out_len, void* hip_stream) {
    clear_error();
    if (!out_len || ((!d_mask || !d_out) && n)) return fail(kNullArgument, "null argument");
    if (cap < alice_codec_rle_bound(n)) return fail(kInvalidBufferSize, "output capacity below alice_codec_rle_bound(n)");
    *out_len = 0;
    if (!n) return kOk;
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    return rle_on_device((const uint8_t*)d_mask, n, (uint8_t*)d_out, out_len, st);
}

int alice_codec_dev_extract_person_rgb(const void* d_mask, uint32_t width, uint32_t height, const uint32_t bbox[4], const void* d_rgb,
                                       void* d_out, uint64_t cap, uint64_t* out_len, void* hip_stream) {
    clear_error();
    if (!bbox || !out_len || !d_mask || !d_rgb) return fail(kNullArgument, "null argument");
    uint64_t total = 0;
    TRY(segment_total(width, height, &total));
    TRY(bbox_indices_fit(width, bbox));
    const uint64_t items = (uint64_t)bbox[2] * bbox[3];
    if (cap < 3 * (unsigned __int128)items) return fail(kInvalidBufferSize, "output capacity below 3 * bbox w * h");
    if (!d_out && items) return fail(kNullArgument, "null argument");
    *out_len = 0;
    if (!items || !total) return kOk;
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    return extract_on_device((const uint8_t*)d_mask, total, (const uint8_t*)d_rgb, 3 * total, width, bbox, (uint8_t*)d_out, out_len, st);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// PART 4: split-stream format (.alc v2; kernels: split.hip)
//
// The front end is v1's (forward_chunk / inverse_chunk: the same symbols); only the entropy stage differs.  Nothing here
// goes through the chain hub: every kernel of this part runs for well under a millisecond per chunk.
// ------------------------------------------------------------------------------------------

namespace {

// fmt: the container (SplitFormat).  Wide (.alc v3) is the same orchestration with two bytes per
// symbol, the wide kernels and lane lengths up to 8192; reversible (.alc v4, section 12) is wide with its own version byte
// and the mirrored inverse.
bool split_lane_ok(uint32_t L, SplitFormat fmt = kFormatSplit) {
    return L >= kSplitMinLane && L <= (is_wide(fmt) ? kSplitWideMaxLane : kSplitMaxLane) && (L & (L - 1u)) == 0u;
}
const char* split_lane_msg(SplitFormat fmt) {
    return is_wide(fmt) ? "lane_symbols must be a power of two in [64, 8192]" : "lane_symbols must be a power of two in [64, 16384]";
}
uint32_t split_blocks(uint64_t n, uint32_t L) { return (uint32_t)((n + 64ull * L - 1) / (64ull * L)); }   // n <= 2^32: at most 2^20

inline void put_u64(uint8_t* p, uint64_t v) { put_u32(p, (uint32_t)v); put_u32(p + 4, (uint32_t)(v >> 32)); }
inline uint64_t get_u64(const uint8_t* p) { return (uint64_t)get_u32(p) | ((uint64_t)get_u32(p + 4) << 32); }

struct SplitHeader {
    uint32_t width = 0, height = 0, frames = 0, lane_symbols = 0;
    uint8_t wavelet = 0;
    SplitFormat fmt = kFormatSplit;   // from the version byte
    int32_t step[3] = {1, 1, 1}, dead_zone[3] = {1, 1, 1};
    uint32_t num_symbols[3] = {0, 0, 0}, n_blocks[3] = {0, 0, 0};
    uint64_t payload_len[3] = {0, 0, 0};
    uint16_t freq[3][256] = {};
};

// Header checks in their fixed order; data: at least min(total_len, kSplitHeaderBytes) readable bytes of a
// container of total_len bytes.
int parse_split_header(const uint8_t* data, uint64_t total_len, SplitHeader& h, ChunkDims* d, int version = 2) {
    if (total_len < kSplitFixedHeaderBytes)
        return fail(kInvalidBitstream, "data too short for the fixed fields: " + std::to_string(total_len) + " bytes (they take " +
                                           std::to_string(kSplitFixedHeaderBytes) + ")");
    if (memcmp(data, "ALCC", 4) != 0) return fail(kInvalidBitstream, "bad magic (expected ALCC)");
    if (data[4] != version)
        return fail(kInvalidBitstream, "unsupported version: " + std::to_string((int)data[4]) + " (expected " + std::to_string(version) + ")");
    h.fmt = format_of_version(version);
    if (data[5] > 2) return fail(kInvalidBitstream, "unknown wavelet type byte: " + std::to_string((int)data[5]));
    h.wavelet = data[5];
    h.width = get_u32(data + 6); h.height = get_u32(data + 10); h.frames = get_u32(data + 14);
    h.lane_symbols = get_u32(data + 18);
    if (!split_lane_ok(h.lane_symbols, h.fmt))
        return fail(kInvalidBitstream, "lane_symbols " + std::to_string(h.lane_symbols) + " is not a power of two in [64, " +
                                           std::to_string(is_wide(h.fmt) ? kSplitWideMaxLane : kSplitMaxLane) + "]");
    if (total_len < kSplitHeaderBytes)
        return fail(kInvalidBitstream, "data too short for the header: " + std::to_string(total_len) + " bytes (minimum " + std::to_string(kSplitHeaderBytes) + ")");
    *d = make_dims(h.width, h.height, h.frames);
    const unsigned __int128 pix = (unsigned __int128)h.width * h.height * h.frames;
    if (pix > UINT64_MAX / 3) return fail(kInvalidBitstream, "dimensions overflow");
    const uint64_t padded = pix == 0 ? 0 : d->padded;
    uint64_t total = kSplitHeaderBytes;
    for (int c = 0; c < 3; ++c) {
        const uint8_t* q = data + kSplitFixedHeaderBytes + (size_t)c * kSplitChannelHeaderBytes;
        const std::string ch = "channel " + std::to_string(c) + ": ";
        h.step[c] = (int32_t)get_u32(q); h.dead_zone[c] = (int32_t)get_u32(q + 4);
        h.num_symbols[c] = get_u32(q + 8); h.n_blocks[c] = get_u32(q + 12);
        h.payload_len[c] = get_u64(q + 16);
        // the encoder writes step = quality_to_step(q) in 1..64 and dead zone = step; a decoder multiplies by the step, so
        // only a step below 1 (no quantiser has one) and a negative dead zone are refused
        if (h.step[c] < 1 || h.dead_zone[c] < 0)
            return fail(kInvalidBitstream, ch + "quantiser step " + std::to_string(h.step[c]) + " / dead zone " + std::to_string(h.dead_zone[c]) +
                                               " (a step is at least 1, a dead zone at least 0)");
        if ((uint64_t)h.num_symbols[c] != padded)
            return fail(kInvalidBitstream, ch + "num_symbols " + std::to_string(h.num_symbols[c]) + " != padded_pixels " + std::to_string(padded));
        if (h.n_blocks[c] != split_blocks(padded, h.lane_symbols))
            return fail(kInvalidBitstream, ch + "n_blocks " + std::to_string(h.n_blocks[c]) + " does not match num_symbols and lane_symbols");
        uint32_t sum = 0;
        for (int i = 0; i < 256; ++i) { h.freq[c][i] = (uint16_t)(q[24 + 2 * i] | (q[25 + 2 * i] << 8)); sum += h.freq[c][i]; }
        if (sum != (padded ? kProbScale : 0u))
            return fail(kInvalidBitstream, ch + "frequencies sum to " + std::to_string(sum) + ", not " + std::to_string(padded ? kProbScale : 0u));
        if (h.payload_len[c] < 132ull * h.n_blocks[c] || h.payload_len[c] > UINT64_MAX / 4)
            return fail(kInvalidBitstream, ch + "payload_len " + std::to_string(h.payload_len[c]) + " cannot hold its directories");
        total += h.payload_len[c];
    }
    if (total != total_len)
        return fail(kInvalidBitstream, "length mismatch: header and payloads are " + std::to_string(total) + " bytes, data is " + std::to_string(total_len));
    return kOk;
}

// the block tables of a whole container in host memory: every block holds its lane directory and the blocks fill the payload
int check_split_directories(const uint8_t* data, const SplitHeader& h) {
    const uint8_t* p = data + kSplitHeaderBytes;
    for (int c = 0; c < 3; ++c) {
        uint64_t sum = 4ull * h.n_blocks[c];
        for (uint32_t b = 0; b < h.n_blocks[c]; ++b) {
            const uint32_t v = get_u32(p + 4ull * b);
            if (v < 128u) return fail(kInvalidBitstream, "channel " + std::to_string(c) + ": block " + std::to_string(b) + " is shorter than its lane directory");
            sum += v;
        }
        if (sum != h.payload_len[c])
            return fail(kInvalidBitstream, "channel " + std::to_string(c) + ": block lengths sum to " + std::to_string(sum) + ", payload_len is " + std::to_string(h.payload_len[c]));
        p += h.payload_len[c];
    }
    return kOk;
}

// device scratch of n_jobs channel jobs of the same symbol count
struct SplitWork {
    int n_jobs = 0;
    uint32_t n_blocks = 0;
    bool wide = false;                // u16 symbols, the wide kernels
    DevBuf jobs, tables, freq, cum, blk_len, blk_off, lane_len, totals, flags;
    std::vector<SplitJob> h;          // edited by the caller between the passes
    // what the asynchronous uploads read: every upload gets a vector of its own that is never touched again, and the
    // destructor drains the stream before they (and the device buffers above, on a caller's NULL stream) are released --
    // also on an error return with kernels still queued
    std::vector<std::vector<SplitJob>> sent;
    std::vector<uint16_t> h_cum, h_freq;
    hipStream_t st = nullptr;
    bool armed = false;
    ~SplitWork() { if (armed) (void)hipStreamSynchronize(st); }
};

int split_work_alloc(SplitWork& w, int n_jobs, uint64_t n, uint32_t L, bool encode, SplitFormat fmt = kFormatSplit) {
    w.n_jobs = n_jobs;
    w.wide = is_wide(fmt);
    w.n_blocks = split_blocks(n, L);
    const size_t nb = w.n_blocks;
    TRY(w.jobs.alloc((size_t)n_jobs * sizeof(SplitJob)));
    TRY(w.tables.alloc((size_t)n_jobs * sizeof(RansTable)));
    TRY(w.freq.alloc((size_t)n_jobs * 256 * sizeof(uint16_t)));
    TRY(w.cum.alloc((size_t)n_jobs * 256 * sizeof(uint16_t)));
    TRY(w.blk_len.alloc((size_t)n_jobs * nb * sizeof(uint32_t)));
    TRY(w.blk_off.alloc((size_t)n_jobs * (nb + 1) * sizeof(unsigned long long)));
    if (encode) TRY(w.lane_len.alloc((size_t)n_jobs * nb * 64 * sizeof(uint16_t)));
    TRY(w.totals.alloc((size_t)n_jobs * sizeof(unsigned long long)));
    TRY(w.flags.alloc((size_t)n_jobs * sizeof(uint32_t)));
    w.h.assign((size_t)n_jobs, SplitJob{});
    for (int j = 0; j < n_jobs; ++j) {
        SplitJob& s = w.h[(size_t)j];
        s.n = n; s.n_blocks = w.n_blocks; s.lane_symbols = L;
        s.table = w.tables.as<RansTable>() + j;
        s.blk_len = w.blk_len.as<uint32_t>() + (size_t)j * nb;
        s.blk_off = w.blk_off.as<unsigned long long>() + (size_t)j * (nb + 1);
        s.lane_len = encode ? w.lane_len.as<uint16_t>() + (size_t)j * nb * 64 : nullptr;
        s.flags = w.flags.as<uint32_t>() + j;
    }
    return kOk;
}

int split_upload_jobs(SplitWork& w, hipStream_t st) {
    w.st = st; w.armed = true;
    w.sent.push_back(w.h);
    HIP_TRY(hipMemcpyAsync(w.jobs.p, w.sent.back().data(), w.h.size() * sizeof(SplitJob), hipMemcpyHostToDevice, st));
    return kOk;
}

// The three channel jobs w.h[first .. first + 3) of the chunk at d_alc (device, h validated): where each payload lies, and
// where its symbols go -- channel c at sym + c * sym_stride (bytes).
void split_chunk_jobs(SplitWork& w, size_t first, const SplitHeader& h, const uint8_t* d_alc, uint8_t* sym, size_t sym_stride) {
    uint64_t off = kSplitHeaderBytes;
    for (int c = 0; c < 3; ++c) {
        SplitJob& s = w.h[first + (size_t)c];
        s.sym = sym + (size_t)c * sym_stride;
        s.stream = (uint8_t*)d_alc + off;
        s.len = h.payload_len[c];
        off += s.len;
    }
}

// Tables from the jobs' histograms (device, n_jobs x 256) and the count pass: totals[j] = payload length of job j.  The
// jobs' symbols (h[j].sym) are set by the caller.  Returns after the stream has drained.
int split_count(SplitWork& w, const uint32_t* d_hist, hipStream_t st, std::vector<uint64_t>& totals, std::vector<uint16_t>* freq_out) {
    launch_split_table(d_hist, w.freq.as<uint16_t>(), w.cum.as<uint16_t>(), w.n_jobs, st);
    for (int j = 0; j < w.n_jobs; ++j)
        launch_rans_table_from_arrays(w.cum.as<uint16_t>() + (size_t)j * 256, w.freq.as<uint16_t>() + (size_t)j * 256, w.tables.as<RansTable>() + j, st);
    TRY(split_upload_jobs(w, st));
    if (w.wide) HIP_TRY(hipMemsetAsync(w.flags.p, 0, (size_t)w.n_jobs * sizeof(uint32_t), st));
    launch_split_count(w.jobs.as<SplitJob>(), w.n_jobs, w.n_blocks, w.wide, st);
    launch_split_scan(w.jobs.as<SplitJob>(), w.n_jobs, false, w.totals.as<unsigned long long>(), st);
    HIP_TRY(hipGetLastError());
    totals.resize((size_t)w.n_jobs);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "totals");
    HIP_TRY(hipMemcpyAsync(totals.data(), w.totals.p, totals.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (freq_out) {
        freq_out->resize((size_t)w.n_jobs * 256);
        HIP_TRY(hipMemcpyAsync(freq_out->data(), w.freq.p, freq_out->size() * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    }
    std::vector<uint32_t> flags;
    if (w.wide) {
        flags.resize((size_t)w.n_jobs);
        HIP_TRY(hipMemcpyAsync(flags.data(), w.flags.p, flags.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    // the residual guard of the wide format: nothing has been written yet, and nothing will be
    for (size_t j = 0; j < flags.size(); ++j)
        if (flags[j] & kSplitWideResidual)
            return fail(kInternal, "stream " + std::to_string(j) + ": a symbol above 255 + 4095 has no version 3 code");
    return kOk;
}

// the write pass, after the caller has pointed every h[j].stream at totals[j] writable bytes
int split_write(SplitWork& w, hipStream_t st) {
    TRY(split_upload_jobs(w, st));
    launch_split_write(w.jobs.as<SplitJob>(), w.n_jobs, w.n_blocks, w.wide, st);
    HIP_TRY(hipGetLastError());
    return kOk;
}

// Decode of the jobs' payloads (h[j].stream / len / sym set by the caller) with the tables of freq (n_jobs x 256, each
// summing to 4096).  Queues the directory scan and the lane decode; split_decode_verdict reads the flags.
// lane_decode: what runs instead of the decode of every block (frame ranges: the planned blocks).
int split_decode_launch(SplitWork& w, const uint16_t* freq, hipStream_t st, const std::function<int()>* lane_decode = nullptr) {
    w.st = st; w.armed = true;
    w.h_freq.assign(freq, freq + (size_t)w.n_jobs * 256);
    freq = w.h_freq.data();
    std::vector<uint16_t>& cum = w.h_cum;
    cum.assign((size_t)w.n_jobs * 256, 0);
    for (int j = 0; j < w.n_jobs; ++j) {
        uint32_t run = 0;
        for (int i = 0; i < 256; ++i) { cum[(size_t)j * 256 + i] = (uint16_t)run; run += freq[(size_t)j * 256 + i]; }
    }
    HIP_TRY(hipMemcpyAsync(w.freq.p, freq, (size_t)w.n_jobs * 256 * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(w.cum.p, cum.data(), cum.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(w.flags.p, 0, (size_t)w.n_jobs * sizeof(uint32_t), st));
    TRY(split_upload_jobs(w, st));
    for (int j = 0; j < w.n_jobs; ++j)
        launch_rans_table_from_arrays(w.cum.as<uint16_t>() + (size_t)j * 256, w.freq.as<uint16_t>() + (size_t)j * 256, w.tables.as<RansTable>() + j, st);
    launch_split_scan(w.jobs.as<SplitJob>(), w.n_jobs, true, nullptr, st);
    if (lane_decode) TRY((*lane_decode)());
    else launch_split_decode(w.jobs.as<SplitJob>(), w.n_jobs, w.n_blocks, w.wide, st);
    HIP_TRY(hipGetLastError());
    return kOk;
}

int split_decode_verdict(SplitWork& w, hipStream_t st) {
    std::vector<uint32_t> flags((size_t)w.n_jobs);
    HIP_TRY(hipMemcpyAsync(flags.data(), w.flags.p, flags.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t j = 0; j < flags.size(); ++j) {
        if (flags[j] & kSplitBadDirectory) return fail(kInvalidBitstream, "stream " + std::to_string(j) + ": block or lane directory does not add up");
        if (flags[j]) return fail(kInvalidBitstream, "stream " + std::to_string(j) + ": a lane failed its end check");
    }
    return kOk;
}

// Whole chunks, in two halves: split_count_chunks runs the forward pass of B equal-shaped chunks at rgb[i] on the device
// (chunk i at quality q[i]), the tables and the count pass, and returns the exact container sizes after the stream has
// drained; split_write_chunks then writes chunk i at outs[i] (device, sizes[i] bytes) and returns after the stream has
// drained.  A budget encode stops after the first half when a quality does not fit.
struct SplitChunkEncode {
    EncodeWork ew;
    std::vector<SplitHeaderDesc> hd;   // (declared before w: w's destructor drains the stream that reads them)
    DevBuf d_hd;
    SplitWork w;
    std::vector<uint64_t> totals;
    std::vector<uint8_t> q;
    std::vector<int32_t> steps, dead_zones;   // a transcode: 3 per chunk, written instead of quality_to_step(q[i])
    uint32_t B = 0, L = 0;
    uint8_t wavelet = 0;
    SplitFormat fmt = kFormatSplit;
};

int split_count_chunks(SplitChunkEncode& e, const RgbLayout* rgb, uint32_t B, const ChunkDims& d, uint8_t wavelet, const uint8_t* q,
                       uint32_t L, hipStream_t st, std::vector<uint64_t>& sizes, SplitFormat fmt = kFormatSplit) {
    EncodeWork& ew = e.ew;
    e.B = B; e.L = L; e.wavelet = wavelet; e.fmt = fmt;
    const bool wide = is_wide(fmt);
    const size_t sb = wide ? 2 : 1;   // bytes per symbol
    e.q.assign(q, q + B);
    ew.d = d; ew.n_chunks = (int)B;
    if (transform_tiles_eligible(d)) TRY(ew.scratch.alloc(forward_scratch_bytes(d)));
    TRY(ew.sym.alloc((size_t)B * 3 * d.padded * sb));
    TRY(ew.hist.alloc((size_t)B * 3 * 256 * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(ew.hist.p, 0, (size_t)B * 3 * 256 * sizeof(uint32_t), st));
    for (uint32_t i = 0; i < B; ++i)
        TRY(forward_chunk(rgb[i], d, wavelet, quality_to_step(q[i]), ew, ew.sym.as<uint8_t>() + (size_t)i * 3 * d.padded * sb,
                          ew.hist.as<uint32_t>() + (size_t)i * 3 * 256, st, wide));
    e.hd.assign(B, SplitHeaderDesc{});
    SplitWork& w = e.w;
    TRY(split_work_alloc(w, (int)(3 * B), d.padded, L, true, fmt));
    for (size_t j = 0; j < 3 * (size_t)B; ++j) w.h[j].sym = ew.sym.as<uint8_t>() + j * d.padded * sb;
    TRY(split_count(w, ew.hist.as<uint32_t>(), st, e.totals, nullptr));
    sizes.resize(B);
    for (uint32_t i = 0; i < B; ++i) sizes[i] = kSplitHeaderBytes + e.totals[3 * i] + e.totals[3 * i + 1] + e.totals[3 * i + 2];
    return kOk;
}

int split_write_chunks(SplitChunkEncode& e, const std::vector<uint8_t*>& outs, hipStream_t st) {
    const uint32_t B = e.B;
    const ChunkDims& d = e.ew.d;
    SplitWork& w = e.w;
    TRY(e.d_hd.alloc((size_t)B * sizeof(SplitHeaderDesc)));
    for (uint32_t i = 0; i < B; ++i) {
        SplitHeaderDesc& h = e.hd[i];
        h.out = outs[i];
        h.width = d.w; h.height = d.h; h.frames = d.f; h.lane_symbols = e.L;
        h.num_symbols = (uint32_t)d.padded; h.n_blocks = w.n_blocks; h.wavelet = e.wavelet;
        h.freq = w.freq.as<uint16_t>() + (size_t)i * 3 * 256;
        uint64_t off = kSplitHeaderBytes;
        for (int c = 0; c < 3; ++c) {
            if (e.steps.empty()) h.step[c] = h.dead_zone[c] = quality_to_step(e.q[i]);
            else { h.step[c] = e.steps[3 * (size_t)i + c]; h.dead_zone[c] = e.dead_zones[3 * (size_t)i + c]; }
            h.payload_len[c] = e.totals[3 * i + c];
            w.h[3 * (size_t)i + c].stream = outs[i] + off;
            off += e.totals[3 * i + c];
        }
    }
    HIP_TRY(hipMemcpyAsync(e.d_hd.p, e.hd.data(), e.hd.size() * sizeof(SplitHeaderDesc), hipMemcpyHostToDevice, st));
    TRY(split_write(w, st));
    launch_split_headers(e.d_hd.as<SplitHeaderDesc>(), (int)B, st);
    if (e.fmt != kFormatSplit) launch_split_header_version(e.d_hd.as<SplitHeaderDesc>(), (int)B, format_version(e.fmt), st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}

// Both halves: place(sizes, outs) is called once the sizes are known and names where each chunk's bytes go (device).
template <typename Place>
int split_encode_chunks(const RgbLayout* rgb, uint32_t B, const ChunkDims& d, uint8_t wavelet, const uint8_t* q, uint32_t L,
                        hipStream_t st, std::vector<uint64_t>& sizes, Place place, SplitFormat fmt = kFormatSplit) {
    SplitChunkEncode e;
    TRY(split_count_chunks(e, rgb, B, d, wavelet, q, L, st, sizes, fmt));
    std::vector<uint8_t*> outs(B, nullptr);
    TRY(place(sizes, outs));
    return split_write_chunks(e, outs, st);
}

// Decode of B equal-shaped chunks: hdr[i] validated, d_alc[i] the chunk's first byte on the device, pixels to rgb[i].
// Returns after the stream has drained, with the verdict of the end checks.
int split_decode_chunks(const SplitHeader* hdr, const uint8_t* const* d_alc, uint32_t B, const ChunkDims& d, const RgbLayout* rgb,
                        hipStream_t st) {
    DecodeWork dw;
    dw.d = d; dw.n_chunks = (int)B;
    const SplitFormat fmt = hdr[0].fmt;   // (one parser, one version per call)
    const bool wide = is_wide(fmt);
    const size_t sb = wide ? 2 : 1;   // bytes per symbol
    TRY(dw.sym.alloc((size_t)B * 3 * d.padded * sb));
    SplitWork w;
    TRY(split_work_alloc(w, (int)(3 * B), d.padded, hdr[0].lane_symbols, false, fmt));
    std::vector<uint16_t> freq((size_t)B * 3 * 256);
    bool any16 = false, any32 = false;
    for (uint32_t i = 0; i < B; ++i) {
        split_chunk_jobs(w, 3 * (size_t)i, hdr[i], d_alc[i], dw.sym.as<uint8_t>() + 3 * (size_t)i * d.padded * sb, d.padded * sb);
        memcpy(&freq[3 * (size_t)i * 256], hdr[i].freq, 3 * 256 * sizeof(uint16_t));
        (inverse_bounds(hdr[i].wavelet, hdr[i].step, wide ? kWideMaxQ : kByteMaxQ).mid16 ? any16 : any32) = true;
    }
    if (transform_tiles_eligible(d)) TRY(dw.scratch_own.alloc(group_scratch_bytes(d, any16, any32)));
    TRY(split_decode_launch(w, freq.data(), st));
    for (uint32_t i = 0; i < B; ++i)
        TRY(inverse_chunk(dw.sym.as<uint8_t>() + (size_t)i * 3 * d.padded * sb, d, hdr[i].wavelet, hdr[i].step, dw.scratch_own.p, dw, rgb[i], st, fmt));
    HIP_TRY(hipGetLastError());
    return split_decode_verdict(w, st);
}

// Chunks a device-resident call works on at a time: as many as keep its symbol buffer at or below 4 GiB (ten 1080p x 64
// chunks).  Every chunk already fills the device on its own, so larger groups gain nothing, and a 32-chunk group (12.7 GB
// of symbols) was measured to DEcode eleven times slower per chunk than groups of eight.
uint32_t split_group(const ChunkDims& d, SplitFormat fmt = kFormatSplit) {
    const uint64_t per_chunk = 3 * d.padded * (is_wide(fmt) ? 2 : 1);
    const uint64_t g = (uint64_t(4) << 30) / (per_chunk ? per_chunk : 1);
    return cap_group((uint32_t)std::min<uint64_t>(std::max<uint64_t>(g, 1), 21845));
}

// ---- the call skeleton of the container entry points of versions 2 to 5: what a call does around its
// groups, written once.  The group bodies (split_encode_chunks, transcode_group, band_encode_chunks, ...) and every check
// of the arguments stay with the entry points. ----

// drains the stream before the buffers declared ahead of it go back to the pool, on every return
struct StreamDrain {
    hipStream_t st;
    explicit StreamDrain(hipStream_t s) : st(s) {}
    ~StreamDrain() { (void)hipStreamSynchronize(st); }
    StreamDrain(const StreamDrain&) = delete;
    StreamDrain& operator=(const StreamDrain&) = delete;
};

// One host buffer in, one host result out.  body(d_src, st, sizes, place) runs one group of one chunk on the uploaded
// input; place(sizes, outs) is the single slot the group writes to.  *out and *out_len are written on success alone, and
// the stream has drained before the device buffers go back to the pool, whichever way the call ends.
template <typename Body>
int host_one_result(const void* src, uint64_t src_len, uint8_t** out, uint64_t* out_len, Body body) {
    hipStream_t st;
    TRY(get_stream(&st));
    DevBuf d_src, d_out;
    StreamDrain drain(st);
    TRY(d_src.alloc(src_len));
    HIP_TRY(hipMemcpyAsync(d_src.p, src, src_len, hipMemcpyHostToDevice, st));
    std::vector<uint64_t> sizes;
    TRY(body(d_src.as<uint8_t>(), st, sizes, [&](const std::vector<uint64_t>& sz, std::vector<uint8_t*>& outs) -> int {
        TRY(d_out.alloc(sz[0]));
        outs[0] = d_out.as<uint8_t>();
        return kOk;
    }));
    std::unique_ptr<uint8_t, decltype(&free)> host(host_result_alloc(sizes[0]), &free);   // freed on every failure below
    if (!host) return fail(kOutOfMemory, "out of host memory");
    TRY(copy_to_host(host.get(), d_out.p, sizes[0], st));
    *out = host.release();
    *out_len = sizes[0];
    return kOk;
}

// The result of a chunk without pixels: fill(p) writes its `bytes` header bytes.  No device is looked for.
template <typename Fill>
int host_header_result(uint64_t bytes, uint8_t** out, uint64_t* out_len, Fill fill) {
    *out = host_result_alloc(bytes);
    if (!*out) return fail(kOutOfMemory, "out of host memory");
    fill(*out);
    *out_len = bytes;
    return kOk;
}

// A validated host container of len bytes to `bytes` of pixels: decode(d_alc, d_rgb, st) runs on the uploaded container.
// *out_len is written once the result has been allocated; a chunk without pixels needs no device.
template <typename Decode>
int host_decode_pixels(const uint8_t* data, uint64_t len, uint64_t bytes, uint8_t** out, uint64_t* out_len, Decode decode) {
    std::unique_ptr<uint8_t, decltype(&free)> host(host_result_alloc(bytes), &free);   // freed on every failure below
    if (!host) return fail(kOutOfMemory, "out of host memory");
    *out_len = bytes;
    if (bytes) {
        hipStream_t st;
        TRY(get_stream(&st));
        DevBuf d_alc, d_rgb;
        StreamDrain drain(st);
        TRY(d_alc.alloc(len));
        TRY(d_rgb.alloc(bytes));
        HIP_TRY(hipMemcpyAsync(d_alc.p, data, len, hipMemcpyHostToDevice, st));
        TRY(decode(d_alc.as<uint8_t>(), d_rgb.p, st));
        TRY(copy_to_host(host.get(), d_rgb.p, bytes, st));
    }
    *out = host.release();
    return kOk;
}

// The headers of n device containers at d_alc + i * alc_stride, read back and validated; nothing else has been queued by
// then.  parse(raw, size, hdr[i], dims) is the format's parser on min(size, header_bytes) bytes (a shorter container leaves
// the rest of its row zero); a chunk without pixels is refused; agree(hdr[0], hdr[i]) compares what the format adds to the
// shape.  d: the shape of all of them; ptr[i]: chunk i's first byte on the device.
template <typename Header, typename Parse, typename Agree>
int read_device_headers(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks, size_t header_bytes, hipStream_t st,
                        Parse parse, Agree agree, const char* agree_msg, std::vector<Header>& hdr, std::vector<const uint8_t*>& ptr,
                        ChunkDims& d) {
    std::vector<uint8_t> raw((size_t)n_chunks * header_bytes, 0);
    for (uint32_t i = 0; i < n_chunks; ++i)
        if (sizes[i])
            HIP_TRY(hipMemcpyAsync(raw.data() + (size_t)i * header_bytes, (const uint8_t*)d_alc + (size_t)i * alc_stride,
                                   std::min<uint64_t>(sizes[i], header_bytes), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    hdr.resize(n_chunks); ptr.resize(n_chunks);
    for (uint32_t i = 0; i < n_chunks; ++i) {
        ChunkDims di{};
        TRY(parse(raw.data() + (size_t)i * header_bytes, sizes[i], hdr[i], di));
        if (di.n_pixels == 0) return fail(kInvalidDimensions, "invalid dimensions");
        if (i == 0) d = di;
        else if (di.w != d.w || di.h != d.h || di.f != d.f || !agree(hdr[0], hdr[i])) return fail(kInvalidDimensions, agree_msg);
        ptr[i] = (const uint8_t*)d_alc + (size_t)i * alc_stride;
    }
    return kOk;
}

// where the chunks of a device call go: chunk first + i at d_out + (first + i) * out_stride, refused before anything of
// the group is written
auto place_strided(void* d_out, uint64_t out_stride, uint32_t first, uint32_t B) {
    return [=](const std::vector<uint64_t>& s, std::vector<uint8_t*>& outs) -> int {
        for (uint32_t i = 0; i < B; ++i) {
            if (s[i] > out_stride)
                return fail(kInvalidBufferSize, "chunk " + std::to_string(first + i) + " needs " + std::to_string(s[i]) +
                                                    " bytes, the output stride is " + std::to_string(out_stride));
            outs[i] = (uint8_t*)d_out + (size_t)(first + i) * out_stride;
        }
        return kOk;
    };
}

// fn(first, B, sz) on chunks [first, first + B) of n_chunks, `group` at a time; a group that succeeds leaves its sizes sz
// in out_sizes (may be null: a decode), so a failure in group k leaves those of the groups before k written.
template <typename Fn>
int for_each_group(uint32_t n_chunks, uint32_t group, uint64_t* out_sizes, Fn fn) {
    for (uint32_t first = 0; first < n_chunks; first += group) {
        const uint32_t B = std::min(group, n_chunks - first);
        std::vector<uint64_t> sz;
        TRY(fn(first, B, sz));
        for (uint32_t i = 0; out_sizes && i < B; ++i) out_sizes[first + i] = sz[i];
    }
    return kOk;
}

// The containers of a device call, after the entry point's own pointers: null argument, empty batch, then a chunk that
// is longer than the stride (a single chunk has no stride to keep).
int check_dev_containers(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks) {
    if (!d_alc || !sizes) return fail(kNullArgument, "null argument");
    if (n_chunks == 0) return fail(kInvalidDimensions, "empty batch");
    for (uint32_t i = 0; i < n_chunks; ++i)
        if (sizes[i] > alc_stride && n_chunks > 1) return fail(kInvalidBufferSize, "chunk " + std::to_string(i) + " is longer than the stride");
    return kOk;
}

void write_empty_split(uint8_t* p, uint8_t wavelet, uint32_t w, uint32_t h, uint32_t f, uint32_t L, int32_t step, uint8_t version = 2) {
    memset(p, 0, kSplitHeaderBytes);
    memcpy(p, "ALCC", 4);
    p[4] = version; p[5] = wavelet;
    put_u32(p + 6, w); put_u32(p + 10, h); put_u32(p + 14, f); put_u32(p + 18, L);
    for (int c = 0; c < 3; ++c) {
        uint8_t* q = p + kSplitFixedHeaderBytes + (size_t)c * kSplitChannelHeaderBytes;
        put_u32(q, (uint32_t)step); put_u32(q + 4, (uint32_t)step);
    }
}

// ---- size prediction and budget encodes of versions 2 and 3 ----
constexpr uint32_t kSplitRefineTrials = 4;   // ALICE_SPLIT_REFINE_TRIALS

// Whole-container brackets of one chunk at the 101 qualities from its 64 x 3 channel payload brackets.
void split_rate_by_quality(const RateChannel* rc, uint64_t* lo, uint64_t* hi) {
    for (int q = 0; q < kQualities; ++q) {
        const RateChannel* c = rc + (size_t)(quality_to_step((uint8_t)q) - 1) * 3;
        lo[q] = kSplitHeaderBytes + c[0].lo + c[1].lo + c[2].lo;
        hi[q] = kSplitHeaderBytes + c[0].hi + c[1].hi + c[2].hi;
    }
}

thread_local std::vector<uint32_t> tl_split_trials;   // alice_codec_test_last_split_trials

// The budget rule of version 2.  q0 = the largest quality in [min_q, max_q] whose upper bound fits.  Above q0 (everywhere
// when there is no q0) the qualities whose bracket straddles the budget are tried from the highest down, one exact size
// (exact(q, &size): forward pass, table, count pass) per quantiser step not tried before, at most kSplitRefineTrials in all;
// the first that fits is chosen.  Otherwise q0; without one, min_q with *fits = 0.  Qualities above 100 act as 100.
template <typename Exact>
int split_choose_quality(const uint64_t* lo, const uint64_t* hi, uint64_t budget, uint8_t min_q, uint8_t max_q, Exact exact,
                         uint8_t* chosen, uint8_t* fits, uint32_t* trials) {
    min_q = std::min<uint8_t>(min_q, 100); max_q = std::min<uint8_t>(max_q, 100);
    int q0 = -1;
    for (int q = max_q; q >= min_q && q0 < 0; --q)
        if (hi[q] <= budget) q0 = q;
    bool tried[65] = {};
    *trials = 0;
    for (int q = max_q; q > q0 && q >= min_q && *trials < kSplitRefineTrials; --q) {
        if (!(lo[q] <= budget && budget < hi[q])) continue;
        const int32_t step = quality_to_step((uint8_t)q);
        if (tried[step]) continue;
        tried[step] = true;
        ++*trials;
        uint64_t size = 0;
        TRY(exact((uint8_t)q, &size));
        if (size <= budget) { *chosen = (uint8_t)q; *fits = 1; return kOk; }
    }
    *chosen = (uint8_t)(q0 >= 0 ? q0 : min_q);
    *fits = q0 >= 0 ? 1 : 0;
    return kOk;
}

// The qualities of n equal-shaped chunks under their budgets: one prediction pass per group, then the refinement trials
// chunk by chunk.  Returns after the stream has drained; nothing is written.  wide: version 3 -- a trial is the wide forward
// pass, the table and the wide count pass, whose residual guard fails the call as it does in an encode.
int split_choose_chunks(const RgbLayout* rgb, uint32_t n, const ChunkDims& d, uint8_t wavelet, uint32_t L, const uint64_t* budgets,
                        uint8_t min_q, uint8_t max_q, uint8_t* chosen, uint8_t* fits, hipStream_t st, SplitFormat fmt = kFormatSplit) {
    tl_split_trials.assign(n, 0u);
    const uint32_t group = split_group(d, fmt);
    uint64_t lo[kQualities], hi[kQualities];
    for (uint32_t first = 0; first < n; first += group) {
        const uint32_t B = std::min(group, n - first);
        std::vector<RateChannel> rc;
        {
            EncodeWork w;
            w.d = d; w.n_chunks = 1;
            if (transform_tiles_eligible(d)) TRY(w.scratch.alloc(forward_scratch_bytes(d)));
            TRY(predict_chunks(rgb + first, B, d, wavelet, w, st, nullptr, rc, L, is_wide(fmt)));
        }
        for (uint32_t i = 0; i < B; ++i) {
            const uint32_t k = first + i;
            split_rate_by_quality(rc.data() + (size_t)i * 192, lo, hi);
            TRY(split_choose_quality(lo, hi, budgets[k], min_q, max_q,
                                     [&](uint8_t q, uint64_t* size) -> int {
                                         SplitChunkEncode e;
                                         std::vector<uint64_t> sz;
                                         TRY(split_count_chunks(e, rgb + k, 1, d, wavelet, &q, L, st, sz, fmt));
                                         *size = sz[0];
                                         return kOk;
                                     },
                                     chosen + k, fits + k, &tl_split_trials[k]));
        }
    }
    return kOk;
}

// n equal-shaped chunks at their layouts -> version 2 (wide: version 3, reversible: version 4) bytes at d_out + i * out_stride, in groups of split_group.
int split_encode_layouts(const RgbLayout* rgb, uint32_t n, const ChunkDims& d, uint8_t wavelet, const uint8_t* q, uint32_t L, void* d_out,
                         uint64_t out_stride, uint64_t* sizes, hipStream_t st, SplitFormat fmt = kFormatSplit) {
    return for_each_group(n, split_group(d, fmt), sizes, [&](uint32_t first, uint32_t B, std::vector<uint64_t>& sz) {
        return split_encode_chunks(rgb + first, B, d, wavelet, q + first, L, st, sz, place_strided(d_out, out_stride, first, B), fmt);
    });
}

// Where the chunks of a device call live.  origins == NULL: n packed chunks back to back at d_frames.  Otherwise chunk i is
// frames [i * f, (i + 1) * f) of the frame_width x frame_height frames at d_frames, cropped to w x h at origins[2i],
// origins[2i + 1] (the rule of region_layouts: a rectangle that leaves the frame is an error before anything is queued).
int split_layouts(const void* d_frames, uint32_t frame_width, uint32_t frame_height, const uint32_t* origins, const ChunkDims& d,
                  uint32_t n, std::vector<RgbLayout>& out) {
    out.resize(n);
    if (!origins) {
        for (uint32_t i = 0; i < n; ++i) out[i] = packed_rgb((const uint8_t*)d_frames + (size_t)i * d.n_pixels * 3, d);
        return kOk;
    }
    uint64_t frame_px = 0;
    TRY(checked_pixel_count(frame_width, frame_height, (uint64_t)d.f * n, &frame_px));
    if (frame_px > UINT64_MAX / 3) return fail(kDimensionOverflow, "dimensions overflow usize");
    const uint64_t row_pitch = 3ull * frame_width, frame_pitch = row_pitch * frame_height;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t x0 = origins[2 * i], y0 = origins[2 * i + 1];
        if (x0 + d.w > frame_width || y0 + d.h > frame_height)
            return fail(kInvalidDimensions, "region " + std::to_string(i) + " at (" + std::to_string(x0) + ", " + std::to_string(y0) +
                                                ") does not lie inside the " + std::to_string(frame_width) + "x" + std::to_string(frame_height) + " frame");
        out[i] = RgbLayout{(uint8_t*)d_frames + (size_t)i * d.f * frame_pitch + y0 * row_pitch + x0 * 3, row_pitch, frame_pitch};
    }
    return kOk;
}

// wavelet, then lane_symbols (0: the default), in the order of the split calls
int check_split_args(uint8_t wavelet_type, uint32_t lane_symbols, uint32_t* L, SplitFormat fmt = kFormatSplit) {
    if (wavelet_type > 2) return fail(kInvalidBitstream, "unknown wavelet type");
    *L = lane_symbols ? lane_symbols : kSplitDefaultLane;
    if (!split_lane_ok(*L, fmt)) return fail(kInvalidDimensions, split_lane_msg(fmt));
    return kOk;
}

// Decode of n device containers into the layouts that layouts_of(dims of the headers, out) names; the headers come to the
// host first, and nothing is queued before they and the layouts have been accepted.
template <typename LayoutsOf>
int split_decode_device(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks, hipStream_t st, LayoutsOf layouts_of,
                        int version = 2) {
    std::vector<SplitHeader> hdr;
    std::vector<const uint8_t*> ptr;
    ChunkDims d{};
    TRY(read_device_headers(d_alc, alc_stride, sizes, n_chunks, kSplitHeaderBytes, st,
                            [&](const uint8_t* raw, uint64_t size, SplitHeader& h, ChunkDims& di) { return parse_split_header(raw, size, h, &di, version); },
                            [](const SplitHeader& h0, const SplitHeader& hi) { return hi.lane_symbols == h0.lane_symbols; },
                            "the chunks of one call must have the same shape and lane_symbols", hdr, ptr, d));
    std::vector<RgbLayout> layouts;
    TRY(layouts_of(d, layouts));
    return for_each_group(n_chunks, split_group(d, format_of_version(version)), nullptr, [&](uint32_t first, uint32_t B, std::vector<uint64_t>&) {
        return split_decode_chunks(hdr.data() + first, ptr.data() + first, B, d, layouts.data() + first, st);
    });
}

}  // namespace

extern "C" {

uint64_t alice_codec_split_stream_bound(uint64_t n, uint32_t lane_symbols) {
    if (!split_lane_ok(lane_symbols) || n > 0xFFFFFFFFull) return 0;
    return (uint64_t)split_blocks(n, lane_symbols) * (4 + 128 + 64 * 4) + 2 * n;
}

int alice_codec_split_normalize(const uint32_t hist[256], uint16_t freq[256]) {
    clear_error();
    if (!hist || !freq) return fail(kNullArgument, "null argument");
    hipStream_t st;
    TRY(get_stream(&st));
    DevBuf dh, df, dc;
    TRY(dh.alloc(256 * 4)); TRY(df.alloc(256 * 2)); TRY(dc.alloc(256 * 2));
    HIP_TRY(hipMemcpyAsync(dh.p, hist, 256 * 4, hipMemcpyHostToDevice, st));
    launch_split_table(dh.as<uint32_t>(), df.as<uint16_t>(), dc.as<uint16_t>(), 1, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(freq, df.p, 256 * 2, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}

static int stage_split_encode(const void* d_symbols, uint64_t n, const uint32_t hist[256], uint32_t lane_symbols, void* d_out,
                              uint64_t cap, uint64_t* out_len, void* hip_stream, SplitFormat fmt) {
    clear_error();
    if ((!d_symbols && n) || !hist || !out_len || (!d_out && cap)) return fail(kNullArgument, "null argument");
    if (!lane_symbols) lane_symbols = kSplitDefaultLane;
    if (!split_lane_ok(lane_symbols, fmt)) return fail(kInvalidDimensions, split_lane_msg(fmt));
    if (n > 0xFFFFFFFFull) return fail(kDimensionOverflow, "more symbols than the header's u32 num_symbols counts");
    uint64_t total = 0;
    for (int i = 0; i < 256; ++i) total += hist[i];
    if (total != n) return fail(kInvalidBufferSize, "the histogram counts " + std::to_string(total) + " symbols, n is " + std::to_string(n));
    *out_len = 0;
    if (!n) return kOk;
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    DevBuf dh;
    TRY(dh.alloc(2 * 256 * 4));
    HIP_TRY(hipMemcpyAsync(dh.p, hist, 256 * 4, hipMemcpyHostToDevice, st));
    // `hist` is the caller's word: the table is normalize(hist) whatever the symbols are, so which of its rows the lanes
    // will meet is counted from the symbols themselves (one pass, nothing inside the lane loop).  A row of frequency 0
    // is the identity step: the count pass and the write pass would both drop the symbol and agree on a payload that
    // decodes to other data.  n < 2^32, so the u32 counts do not wrap.
    uint32_t* const d_used = dh.as<uint32_t>() + 256;
    HIP_TRY(hipMemsetAsync(d_used, 0, 256 * 4, st));
    if (is_wide(fmt)) launch_histogram_wide((const uint16_t*)d_symbols, n, d_used, st);
    else launch_histogram((const uint8_t*)d_symbols, n, d_used, st);
    HIP_TRY(hipGetLastError());
    uint32_t used[256];
    HIP_TRY(hipMemcpyAsync(used, d_used, sizeof(used), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int s = 0; s < 256; ++s)
        if (used[s] && !hist[s])
            return fail(kInvalidBufferSize, "hist[" + std::to_string(s) + "] is 0 but the data holds symbol " + std::to_string(s) +
                                                " (count " + std::to_string(used[s]) + ")" +
                                                (is_wide(fmt) && s == 255 ? ": 255 is the escape, every z >= 255" : ""));
    SplitWork w;
    TRY(split_work_alloc(w, 1, n, lane_symbols, true, fmt));
    w.h[0].sym = (const uint8_t*)d_symbols;
    std::vector<uint64_t> totals;
    TRY(split_count(w, dh.as<uint32_t>(), st, totals, nullptr));
    if (totals[0] > cap)
        return fail(kInvalidBufferSize, "the stream needs " + std::to_string(totals[0]) + " bytes, capacity is " + std::to_string(cap) +
                                            (is_wide(fmt) ? " (alice_codec_wide_stream_bound gives the worst case)"
                                                  : " (alice_codec_split_stream_bound gives the worst case)"));
    w.h[0].stream = (uint8_t*)d_out;
    TRY(split_write(w, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out_len = totals[0];
    return kOk;
}

int alice_codec_dev_split_encode(const void* d_symbols, uint64_t n, const uint32_t hist[256], uint32_t lane_symbols, void* d_out,
                                 uint64_t cap, uint64_t* out_len, void* hip_stream) {
    return stage_split_encode(d_symbols, n, hist, lane_symbols, d_out, cap, out_len, hip_stream, kFormatSplit);
}

static int stage_split_decode(const void* d_stream, uint64_t len, const uint16_t freq[256], uint32_t lane_symbols, void* d_symbols,
                              uint64_t n, void* hip_stream, SplitFormat fmt) {
    clear_error();
    if ((!d_stream && len) || !freq || (!d_symbols && n)) return fail(kNullArgument, "null argument");
    if (!lane_symbols) lane_symbols = kSplitDefaultLane;
    if (!split_lane_ok(lane_symbols, fmt)) return fail(kInvalidDimensions, split_lane_msg(fmt));
    if (n > 0xFFFFFFFFull) return fail(kDimensionOverflow, "more symbols than the header's u32 num_symbols counts");
    uint32_t sum = 0;
    for (int i = 0; i < 256; ++i) sum += freq[i];
    if (sum != (n ? kProbScale : 0u)) return fail(kInvalidBitstream, "frequencies sum to " + std::to_string(sum) + ", not " + std::to_string(n ? kProbScale : 0u));
    if (!n) return len == 0 ? (int)kOk : fail(kInvalidBitstream, "an empty channel has no payload");
    if (len < 132ull * split_blocks(n, lane_symbols)) return fail(kInvalidBitstream, "the payload cannot hold its directories");
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    SplitWork w;
    TRY(split_work_alloc(w, 1, n, lane_symbols, false, fmt));
    w.h[0].sym = (const uint8_t*)d_symbols;
    w.h[0].stream = (uint8_t*)d_stream;
    w.h[0].len = len;
    TRY(split_decode_launch(w, freq, st));
    return split_decode_verdict(w, st);
}

int alice_codec_dev_split_decode(const void* d_stream, uint64_t len, const uint16_t freq[256], uint32_t lane_symbols, void* d_symbols,
                                 uint64_t n, void* hip_stream) {
    return stage_split_decode(d_stream, len, freq, lane_symbols, d_symbols, n, hip_stream, kFormatSplit);
}

static int container_info(const uint8_t* data, uint64_t len, AliceSplitInfo* info, int version) {
    clear_error();
    if (!data || !info) return fail(kNullArgument, "null argument");
    SplitHeader h;
    ChunkDims d{};
    TRY(parse_split_header(data, len, h, &d, version));
    TRY(check_split_directories(data, h));
    memset(info, 0, sizeof(*info));
    info->width = h.width; info->height = h.height; info->frames = h.frames;
    info->lane_symbols = h.lane_symbols; info->wavelet = h.wavelet;
    for (int c = 0; c < 3; ++c) {
        info->quant_step[c] = h.step[c]; info->dead_zone[c] = h.dead_zone[c];
        info->num_symbols[c] = h.num_symbols[c]; info->n_blocks[c] = h.n_blocks[c];
        info->payload_len[c] = h.payload_len[c];
    }
    return kOk;
}

int alice_codec_split_info(const uint8_t* data, uint64_t len, AliceSplitInfo* info) { return container_info(data, len, info, 2); }

static uint8_t* container_encode(const FrameEncoder* encoder, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                                 uint32_t frames, uint32_t lane_symbols, uint64_t* out_len, SplitFormat fmt) {
    clear_error();
    if (!encoder || !rgb || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    auto run = [&](uint8_t** out) -> int {
        uint64_t n_pixels = 0;
        TRY(checked_pixel_count(width, height, frames, &n_pixels));
        if (n_pixels == 0 && rgb_len != 0) return fail(kInvalidBufferSize, "buffer size mismatch: expected 0, got " + std::to_string(rgb_len));
        ChunkDims d{};
        EncodedChunk* none = nullptr;
        if (n_pixels) TRY(validate_encode_many(encoder, rgb, rgb_len, width, height, frames, 1, &none, &d));
        const uint32_t L = lane_symbols ? lane_symbols : kSplitDefaultLane;
        if (!split_lane_ok(L, fmt)) return fail(kInvalidDimensions, split_lane_msg(fmt));
        if (n_pixels == 0)
            return host_header_result(kSplitHeaderBytes, out, out_len, [&](uint8_t* p) {
                write_empty_split(p, encoder->wavelet, width, height, frames, L, quality_to_step(encoder->quality), format_version(fmt));
            });
        return host_one_result(rgb, n_pixels * 3, out, out_len, [&](const uint8_t* d_rgb, hipStream_t st, std::vector<uint64_t>& sizes, auto place) {
            const RgbLayout layout = packed_rgb(d_rgb, d);
            return split_encode_chunks(&layout, 1, d, encoder->wavelet, &encoder->quality, L, st, sizes, place, fmt);
        });
    };
    uint8_t* out = nullptr;
    return run(&out) == kOk ? out : nullptr;
}

uint8_t* alice_codec_encode_split(const FrameEncoder* encoder, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                                  uint32_t frames, uint32_t lane_symbols, uint64_t* out_len) {
    return container_encode(encoder, rgb, rgb_len, width, height, frames, lane_symbols, out_len, kFormatSplit);
}

static uint8_t* container_decode(const uint8_t* data, uint64_t len, uint64_t* out_len, int version) {
    clear_error();
    if (!data || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    auto run = [&](uint8_t** out) -> int {
        SplitHeader h;
        ChunkDims d{};
        TRY(parse_split_header(data, len, h, &d, version));
        TRY(check_split_directories(data, h));
        return host_decode_pixels(data, len, (uint64_t)h.width * h.height * h.frames * 3, out, out_len,
                                  [&](const uint8_t* d_alc, void* d_rgb, hipStream_t st) {
                                      const RgbLayout layout = packed_rgb(d_rgb, d);
                                      return split_decode_chunks(&h, &d_alc, 1, d, &layout, st);
                                  });
    };
    uint8_t* out = nullptr;
    return run(&out) == kOk ? out : nullptr;
}

uint8_t* alice_codec_decode_split(const uint8_t* data, uint64_t len, uint64_t* out_len) { return container_decode(data, len, out_len, 2); }

static int container_dev_encode(const void* d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                uint8_t wavelet_type, uint8_t quality, const uint8_t* qualities, uint32_t lane_symbols, void* d_out,
                                uint64_t out_stride, uint64_t* sizes, void* hip_stream, SplitFormat fmt) {
    clear_error();
    if (!d_rgb || !d_out || !sizes) return fail(kNullArgument, "null argument");
    if (wavelet_type > 2) return fail(kInvalidBitstream, "unknown wavelet type");
    ChunkDims d{};
    TRY(chunk_dims(width, height, frames, &d, n_chunks));
    const uint32_t L = lane_symbols ? lane_symbols : kSplitDefaultLane;
    if (!split_lane_ok(L, fmt)) return fail(kInvalidDimensions, split_lane_msg(fmt));
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    std::vector<RgbLayout> layouts(n_chunks);
    std::vector<uint8_t> q(n_chunks);
    for (uint32_t i = 0; i < n_chunks; ++i) {
        layouts[i] = packed_rgb((const uint8_t*)d_rgb + (size_t)i * d.n_pixels * 3, d);
        q[i] = qualities ? qualities[i] : quality;
    }
    return split_encode_layouts(layouts.data(), n_chunks, d, wavelet_type, q.data(), L, d_out, out_stride, sizes, st, fmt);
}

int alice_codec_dev_encode_split(const void* d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                 uint8_t wavelet_type, uint8_t quality, const uint8_t* qualities, uint32_t lane_symbols, void* d_out,
                                 uint64_t out_stride, uint64_t* sizes, void* hip_stream) {
    return container_dev_encode(d_rgb, width, height, frames, n_chunks, wavelet_type, quality, qualities, lane_symbols, d_out, out_stride,
                                sizes, hip_stream, kFormatSplit);
}

static int container_dev_decode(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks, void* d_rgb_out,
                                void* hip_stream, int version) {
    clear_error();
    if (!d_rgb_out) return fail(kNullArgument, "null argument");
    TRY(check_dev_containers(d_alc, alc_stride, sizes, n_chunks));
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    return split_decode_device(d_alc, alc_stride, sizes, n_chunks, st, [&](const ChunkDims& d, std::vector<RgbLayout>& out) {
        return split_layouts(d_rgb_out, 0, 0, nullptr, d, n_chunks, out);
    }, version);
}

int alice_codec_dev_decode_split(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks, void* d_rgb_out,
                                 void* hip_stream) {
    return container_dev_decode(d_alc, alc_stride, sizes, n_chunks, d_rgb_out, hip_stream, 2);
}

// ---- version 3: the wide container.  The same paths with the wide flag set. ----

uint64_t alice_codec_wide_stream_bound(uint64_t n, uint32_t lane_symbols) {
    if (!split_lane_ok(lane_symbols, kFormatWide) || n > 0xFFFFFFFFull) return 0;
    return (uint64_t)split_blocks(n, lane_symbols) * (4 + 128 + 64 * 4) + 4 * n;
}

int alice_codec_dev_wide_encode(const void* d_symbols, uint64_t n, const uint32_t hist[256], uint32_t lane_symbols, void* d_out,
                                uint64_t cap, uint64_t* out_len, void* hip_stream) {
    return stage_split_encode(d_symbols, n, hist, lane_symbols, d_out, cap, out_len, hip_stream, kFormatWide);
}

int alice_codec_dev_wide_decode(const void* d_stream, uint64_t len, const uint16_t freq[256], uint32_t lane_symbols, void* d_symbols,
                                uint64_t n, void* hip_stream) {
    return stage_split_decode(d_stream, len, freq, lane_symbols, d_symbols, n, hip_stream, kFormatWide);
}

int alice_codec_wide_info(const uint8_t* data, uint64_t len, AliceSplitInfo* info) { return container_info(data, len, info, 3); }

uint8_t* alice_codec_encode_wide(const FrameEncoder* encoder, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                                 uint32_t frames, uint32_t lane_symbols, uint64_t* out_len) {
    return container_encode(encoder, rgb, rgb_len, width, height, frames, lane_symbols, out_len, kFormatWide);
}

uint8_t* alice_codec_decode_wide(const uint8_t* data, uint64_t len, uint64_t* out_len) { return container_decode(data, len, out_len, 3); }

int alice_codec_dev_encode_wide(const void* d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                uint8_t wavelet_type, uint8_t quality, const uint8_t* qualities, uint32_t lane_symbols, void* d_out,
                                uint64_t out_stride, uint64_t* sizes, void* hip_stream) {
    return container_dev_encode(d_rgb, width, height, frames, n_chunks, wavelet_type, quality, qualities, lane_symbols, d_out, out_stride,
                                sizes, hip_stream, kFormatWide);
}

int alice_codec_dev_decode_wide(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks, void* d_rgb_out,
                                void* hip_stream) {
    return container_dev_decode(d_alc, alc_stride, sizes, n_chunks, d_rgb_out, hip_stream, 3);
}

// ---- versions 2 and 3: size prediction, budget encodes, regions of device frames.  One body per
// call, the container as an argument (wide: version 3). ----

static int container_predict_sizes(uint8_t wavelet_type, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                                   uint32_t frames, uint32_t lane_symbols, uint64_t lo[101], uint64_t hi[101], SplitFormat fmt) {
    clear_error();
    if (!lo || !hi || (!rgb && rgb_len)) return fail(kNullArgument, "null argument");
    uint64_t n_pixels = 0;
    TRY(checked_pixel_count(width, height, frames, &n_pixels));
    if (n_pixels == 0 && rgb_len != 0) return fail(kInvalidBufferSize, "buffer size mismatch: expected 0, got " + std::to_string(rgb_len));
    const FrameEncoder enc{0, wavelet_type};
    ChunkDims d{};
    EncodedChunk* none = nullptr;
    if (n_pixels) TRY(validate_encode_many(&enc, rgb, rgb_len, width, height, frames, 1, &none, &d));
    uint32_t L = 0;
    TRY(check_split_args(wavelet_type, lane_symbols, &L, fmt));
    if (n_pixels == 0) {   // an empty chunk is its header at every quality
        for (int q = 0; q < kQualities; ++q) lo[q] = hi[q] = kSplitHeaderBytes;
        return kOk;
    }
    hipStream_t st;
    TRY(get_stream(&st));
    DevBuf d_rgb;
    EncodeWork w;
    w.d = d; w.n_chunks = 1;
    if (transform_tiles_eligible(d)) TRY(w.scratch.alloc(forward_scratch_bytes(d)));
    TRY(d_rgb.alloc(n_pixels * 3));
    HIP_TRY(hipMemcpyAsync(d_rgb.p, rgb, n_pixels * 3, hipMemcpyHostToDevice, st));
    const RgbLayout layout = packed_rgb(d_rgb.p, d);
    std::vector<RateChannel> rc;
    TRY(predict_chunks(&layout, 1, d, wavelet_type, w, st, nullptr, rc, L, is_wide(fmt)));
    split_rate_by_quality(rc.data(), lo, hi);
    return kOk;
}

int alice_codec_predict_split_sizes(uint8_t wavelet_type, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                                    uint32_t frames, uint32_t lane_symbols, uint64_t lo[101], uint64_t hi[101]) {
    return container_predict_sizes(wavelet_type, rgb, rgb_len, width, height, frames, lane_symbols, lo, hi, kFormatSplit);
}

int alice_codec_predict_wide_sizes(uint8_t wavelet_type, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                                   uint32_t frames, uint32_t lane_symbols, uint64_t lo[101], uint64_t hi[101]) {
    return container_predict_sizes(wavelet_type, rgb, rgb_len, width, height, frames, lane_symbols, lo, hi, kFormatWide);
}

// d_step_hist: [chunk][step - 1][channel][256] u32 on the device, or null
static int container_dev_predict_sizes(const void* d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                       uint8_t wavelet_type, uint32_t lane_symbols, uint64_t* lo, uint64_t* hi, void* d_step_hist,
                                       void* hip_stream, SplitFormat fmt) {
    clear_error();
    if (!d_rgb || !lo || !hi) return fail(kNullArgument, "null argument");
    ChunkDims d{};
    TRY(chunk_dims(width, height, frames, &d, n_chunks));
    uint32_t L = 0;
    TRY(check_split_args(wavelet_type, lane_symbols, &L, fmt));
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    EncodeWork w;
    w.d = d; w.n_chunks = 1;
    if (transform_tiles_eligible(d)) TRY(w.scratch.alloc(forward_scratch_bytes(d)));
    std::vector<RgbLayout> layouts;
    TRY(split_layouts(d_rgb, 0, 0, nullptr, d, n_chunks, layouts));
    const uint32_t group = split_group(d, fmt);
    for (uint32_t first = 0; first < n_chunks; first += group) {
        const uint32_t B = std::min(group, n_chunks - first);
        std::vector<RateChannel> rc;
        uint32_t* sh = d_step_hist ? (uint32_t*)d_step_hist + (size_t)first * 64 * 3 * 256 : nullptr;
        TRY(predict_chunks(layouts.data() + first, B, d, wavelet_type, w, st, sh, rc, L, is_wide(fmt)));
        for (uint32_t i = 0; i < B; ++i)
            split_rate_by_quality(rc.data() + (size_t)i * 192, lo + (size_t)(first + i) * kQualities, hi + (size_t)(first + i) * kQualities);
    }
    return kOk;
}

int alice_codec_dev_predict_split_sizes(const void* d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                        uint8_t wavelet_type, uint32_t lane_symbols, uint64_t* lo, uint64_t* hi, void* hip_stream) {
    return container_dev_predict_sizes(d_rgb, width, height, frames, n_chunks, wavelet_type, lane_symbols, lo, hi, nullptr, hip_stream, kFormatSplit);
}

int alice_codec_dev_predict_wide_sizes(const void* d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                       uint8_t wavelet_type, uint32_t lane_symbols, uint64_t* lo, uint64_t* hi, void* d_step_hist,
                                       void* hip_stream) {
    return container_dev_predict_sizes(d_rgb, width, height, frames, n_chunks, wavelet_type, lane_symbols, lo, hi, d_step_hist, hip_stream, kFormatWide);
}

static uint8_t* container_encode_to_size(uint8_t wavelet_type, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                                         uint32_t frames, uint32_t lane_symbols, uint64_t max_bytes, uint8_t min_q, uint8_t max_q,
                                         uint8_t* chosen_q, uint8_t* fits, uint64_t* out_len, SplitFormat fmt) {
    clear_error();
    if (!chosen_q || !fits || !out_len || (!rgb && rgb_len)) { fail(kNullArgument, "null argument"); return nullptr; }
    auto run = [&](uint8_t** out) -> int {
        uint64_t n_pixels = 0;
        TRY(checked_pixel_count(width, height, frames, &n_pixels));
        if (n_pixels == 0 && rgb_len != 0) return fail(kInvalidBufferSize, "buffer size mismatch: expected 0, got " + std::to_string(rgb_len));
        const FrameEncoder enc{0, wavelet_type};
        ChunkDims d{};
        EncodedChunk* none = nullptr;
        if (n_pixels) TRY(validate_encode_many(&enc, rgb, rgb_len, width, height, frames, 1, &none, &d));
        uint32_t L = 0;
        TRY(check_split_args(wavelet_type, lane_symbols, &L, fmt));
        TRY(check_quality_range(min_q, max_q));
        if (n_pixels == 0) {
            uint64_t lo[kQualities], hi[kQualities];
            for (int q = 0; q < kQualities; ++q) lo[q] = hi[q] = kSplitHeaderBytes;
            tl_split_trials.assign(1, 0u);
            TRY(split_choose_quality(lo, hi, max_bytes, min_q, max_q, [](uint8_t, uint64_t*) -> int { return kOk; }, chosen_q, fits,
                                     &tl_split_trials[0]));
            return host_header_result(kSplitHeaderBytes, out, out_len, [&](uint8_t* p) {
                write_empty_split(p, wavelet_type, width, height, frames, L, quality_to_step(*chosen_q), format_version(fmt));
            });
        }
        // (*chosen_q and *fits are the chooser's own outputs, here as in the branch above: written before the encode)
        return host_one_result(rgb, n_pixels * 3, out, out_len, [&](const uint8_t* d_rgb, hipStream_t st, std::vector<uint64_t>& sizes, auto place) -> int {
            const RgbLayout layout = packed_rgb(d_rgb, d);
            TRY(split_choose_chunks(&layout, 1, d, wavelet_type, L, &max_bytes, min_q, max_q, chosen_q, fits, st, fmt));
            return split_encode_chunks(&layout, 1, d, wavelet_type, chosen_q, L, st, sizes, place, fmt);
        });
    };
    uint8_t* out = nullptr;
    return run(&out) == kOk ? out : nullptr;
}

uint8_t* alice_codec_encode_split_to_size(uint8_t wavelet_type, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                                          uint32_t frames, uint32_t lane_symbols, uint64_t max_bytes, uint8_t min_q, uint8_t max_q,
                                          uint8_t* chosen_q, uint8_t* fits, uint64_t* out_len) {
    return container_encode_to_size(wavelet_type, rgb, rgb_len, width, height, frames, lane_symbols, max_bytes, min_q, max_q, chosen_q,
                                    fits, out_len, kFormatSplit);
}

uint8_t* alice_codec_encode_wide_to_size(uint8_t wavelet_type, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                                         uint32_t frames, uint32_t lane_symbols, uint64_t max_bytes, uint8_t min_q, uint8_t max_q,
                                         uint8_t* chosen_q, uint8_t* fits, uint64_t* out_len) {
    return container_encode_to_size(wavelet_type, rgb, rgb_len, width, height, frames, lane_symbols, max_bytes, min_q, max_q, chosen_q,
                                    fits, out_len, kFormatWide);
}

static int container_dev_encode_regions(const void* d_frames, uint32_t frame_width, uint32_t frame_height, const uint32_t* origins,
                                        uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks, uint8_t wavelet_type,
                                        uint8_t quality, const uint8_t* qualities, uint32_t lane_symbols, void* d_out,
                                        uint64_t out_stride, uint64_t* sizes, void* hip_stream, SplitFormat fmt) {
    clear_error();
    if (!d_frames || !origins || !d_out || !sizes) return fail(kNullArgument, "null argument");
    ChunkDims d{};
    TRY(chunk_dims(width, height, frames, &d, n_chunks));
    std::vector<RgbLayout> layouts;
    TRY(split_layouts(d_frames, frame_width, frame_height, origins, d, n_chunks, layouts));
    uint32_t L = 0;
    TRY(check_split_args(wavelet_type, lane_symbols, &L, fmt));
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    std::vector<uint8_t> q(n_chunks);
    for (uint32_t i = 0; i < n_chunks; ++i) q[i] = qualities ? qualities[i] : quality;
    return split_encode_layouts(layouts.data(), n_chunks, d, wavelet_type, q.data(), L, d_out, out_stride, sizes, st, fmt);
}

int alice_codec_dev_encode_split_regions(const void* d_frames, uint32_t frame_width, uint32_t frame_height, const uint32_t* origins,
                                         uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks, uint8_t wavelet_type,
                                         uint8_t quality, const uint8_t* qualities, uint32_t lane_symbols, void* d_out,
                                         uint64_t out_stride, uint64_t* sizes, void* hip_stream) {
    return container_dev_encode_regions(d_frames, frame_width, frame_height, origins, width, height, frames, n_chunks, wavelet_type, quality,
                                        qualities, lane_symbols, d_out, out_stride, sizes, hip_stream, kFormatSplit);
}

int alice_codec_dev_encode_wide_regions(const void* d_frames, uint32_t frame_width, uint32_t frame_height, const uint32_t* origins,
                                        uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks, uint8_t wavelet_type,
                                        uint8_t quality, const uint8_t* qualities, uint32_t lane_symbols, void* d_out,
                                        uint64_t out_stride, uint64_t* sizes, void* hip_stream) {
    return container_dev_encode_regions(d_frames, frame_width, frame_height, origins, width, height, frames, n_chunks, wavelet_type, quality,
                                        qualities, lane_symbols, d_out, out_stride, sizes, hip_stream, kFormatWide);
}

static int container_dev_decode_regions(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks,
                                        void* d_frames_out, uint32_t frame_width, uint32_t frame_height, const uint32_t* origins,
                                        void* hip_stream, int version) {
    clear_error();
    if (!d_alc || !sizes || !d_frames_out || !origins) return fail(kNullArgument, "null argument");
    if (n_chunks == 0) return fail(kInvalidDimensions, "empty batch");
    for (uint32_t i = 0; i < n_chunks; ++i) {
        if (sizes[i] > alc_stride && n_chunks > 1) return fail(kInvalidBufferSize, "chunk " + std::to_string(i) + " is longer than the stride");
        if (origins[2 * i] >= frame_width || origins[2 * i + 1] >= frame_height)   // (the whole rectangle once the headers are read)
            return fail(kInvalidDimensions, "region " + std::to_string(i) + " starts outside the " + std::to_string(frame_width) + "x" +
                                                std::to_string(frame_height) + " frame");
    }
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    return split_decode_device(d_alc, alc_stride, sizes, n_chunks, st, [&](const ChunkDims& d, std::vector<RgbLayout>& out) {
        return split_layouts(d_frames_out, frame_width, frame_height, origins, d, n_chunks, out);
    }, version);
}

int alice_codec_dev_decode_split_regions(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks,
                                         void* d_frames_out, uint32_t frame_width, uint32_t frame_height, const uint32_t* origins,
                                         void* hip_stream) {
    return container_dev_decode_regions(d_alc, alc_stride, sizes, n_chunks, d_frames_out, frame_width, frame_height, origins, hip_stream, 2);
}

int alice_codec_dev_decode_wide_regions(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks,
                                        void* d_frames_out, uint32_t frame_width, uint32_t frame_height, const uint32_t* origins,
                                        void* hip_stream) {
    return container_dev_decode_regions(d_alc, alc_stride, sizes, n_chunks, d_frames_out, frame_width, frame_height, origins, hip_stream, 3);
}

static int container_dev_encode_to_budget(const void* d_frames, uint32_t frame_width, uint32_t frame_height, const uint32_t* origins,
                                          uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks, uint8_t wavelet_type,
                                          uint32_t lane_symbols, const uint64_t* budgets, uint8_t min_q, uint8_t max_q, uint8_t* chosen,
                                          uint8_t* fits, void* d_out, uint64_t out_stride, uint64_t* sizes, void* hip_stream, SplitFormat fmt) {
    clear_error();
    if (!d_frames || !budgets || !chosen || !fits || !d_out || !sizes) return fail(kNullArgument, "null argument");
    ChunkDims d{};
    TRY(chunk_dims(width, height, frames, &d, n_chunks));
    std::vector<RgbLayout> layouts;
    TRY(split_layouts(d_frames, frame_width, frame_height, origins, d, n_chunks, layouts));
    uint32_t L = 0;
    TRY(check_split_args(wavelet_type, lane_symbols, &L, fmt));
    TRY(check_quality_range(min_q, max_q));
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    // the choices reach the caller only with the bytes: a failed call leaves chosen / fits / sizes as they were
    std::vector<uint8_t> q(n_chunks), ok(n_chunks);
    std::vector<uint64_t> sz(n_chunks);
    TRY(split_choose_chunks(layouts.data(), n_chunks, d, wavelet_type, L, budgets, min_q, max_q, q.data(), ok.data(), st, fmt));
    TRY(split_encode_layouts(layouts.data(), n_chunks, d, wavelet_type, q.data(), L, d_out, out_stride, sz.data(), st, fmt));
    for (uint32_t i = 0; i < n_chunks; ++i) { chosen[i] = q[i]; fits[i] = ok[i]; sizes[i] = sz[i]; }
    return kOk;
}

int alice_codec_dev_encode_split_to_budget(const void* d_frames, uint32_t frame_width, uint32_t frame_height, const uint32_t* origins,
                                           uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks, uint8_t wavelet_type,
                                           uint32_t lane_symbols, const uint64_t* budgets, uint8_t min_q, uint8_t max_q, uint8_t* chosen,
                                           uint8_t* fits, void* d_out, uint64_t out_stride, uint64_t* sizes, void* hip_stream) {
    return container_dev_encode_to_budget(d_frames, frame_width, frame_height, origins, width, height, frames, n_chunks, wavelet_type,
                                          lane_symbols, budgets, min_q, max_q, chosen, fits, d_out, out_stride, sizes, hip_stream, kFormatSplit);
}

int alice_codec_dev_encode_wide_to_budget(const void* d_frames, uint32_t frame_width, uint32_t frame_height, const uint32_t* origins,
                                          uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks, uint8_t wavelet_type,
                                          uint32_t lane_symbols, const uint64_t* budgets, uint8_t min_q, uint8_t max_q, uint8_t* chosen,
                                          uint8_t* fits, void* d_out, uint64_t out_stride, uint64_t* sizes, void* hip_stream) {
    return container_dev_encode_to_budget(d_frames, frame_width, frame_height, origins, width, height, frames, n_chunks, wavelet_type,
                                          lane_symbols, budgets, min_q, max_q, chosen, fits, d_out, out_stride, sizes, hip_stream, kFormatWide);
}

// ---- version 4: the reversible container.  The wide paths with the format set to reversible: the
// version byte and the inverse launcher are all that differ. ----

uint8_t* alice_codec_encode_reversible(const FrameEncoder* encoder, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                                       uint32_t frames, uint32_t lane_symbols, uint64_t* out_len) {
    return container_encode(encoder, rgb, rgb_len, width, height, frames, lane_symbols, out_len, kFormatReversible);
}

uint8_t* alice_codec_decode_reversible(const uint8_t* data, uint64_t len, uint64_t* out_len) { return container_decode(data, len, out_len, 4); }

int alice_codec_reversible_info(const uint8_t* data, uint64_t len, AliceSplitInfo* info) { return container_info(data, len, info, 4); }

int alice_codec_dev_encode_reversible(const void* d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                      uint8_t wavelet_type, uint8_t quality, const uint8_t* qualities, uint32_t lane_symbols, void* d_out,
                                      uint64_t out_stride, uint64_t* sizes, void* hip_stream) {
    return container_dev_encode(d_rgb, width, height, frames, n_chunks, wavelet_type, quality, qualities, lane_symbols, d_out, out_stride,
                                sizes, hip_stream, kFormatReversible);
}

int alice_codec_dev_decode_reversible(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks, void* d_rgb_out,
                                      void* hip_stream) {
    return container_dev_decode(d_alc, alc_stride, sizes, n_chunks, d_rgb_out, hip_stream, 4);
}

int alice_codec_dev_encode_reversible_regions(const void* d_frames, uint32_t frame_width, uint32_t frame_height, const uint32_t* origins,
                                              uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks, uint8_t wavelet_type,
                                              uint8_t quality, const uint8_t* qualities, uint32_t lane_symbols, void* d_out,
                                              uint64_t out_stride, uint64_t* sizes, void* hip_stream) {
    return container_dev_encode_regions(d_frames, frame_width, frame_height, origins, width, height, frames, n_chunks, wavelet_type, quality,
                                        qualities, lane_symbols, d_out, out_stride, sizes, hip_stream, kFormatReversible);
}

int alice_codec_dev_decode_reversible_regions(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks,
                                              void* d_frames_out, uint32_t frame_width, uint32_t frame_height, const uint32_t* origins,
                                              void* hip_stream) {
    return container_dev_decode_regions(d_alc, alc_stride, sizes, n_chunks, d_frames_out, frame_width, frame_height, origins, hip_stream, 4);
}

uint32_t alice_codec_test_last_split_trials(uint32_t* per_chunk, uint32_t cap) {
    const uint32_t n = (uint32_t)tl_split_trials.size();
    for (uint32_t i = 0; i < n && i < cap && per_chunk; ++i) per_chunk[i] = tl_split_trials[i];
    return n;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// PART 5: quality control (kernel: quality.hip)
//
// The lane coders of versions 2 to 4 are lossless, so a decode returns inverse_chunk(forward_chunk(q)): a trial is that
// transform pair into pool scratch plus launch_rgb_sse against the source.  Nothing here touches split.hip or the chain hub.
// ------------------------------------------------------------------------------------------

namespace {

static_assert(ALICE_QUALITY_MAX_TRIALS == 8, "2 + ceil(log2(63)) trials for the 64 steps");
thread_local std::vector<uint32_t> tl_quality_trials;   // alice_codec_test_last_quality_trials

int check_format_byte(uint8_t format, SplitFormat* fmt) {
    if (format < 2 || format > 4) return fail(kInvalidBitstream, "unknown format byte: " + std::to_string((int)format) + " (2, 3 or 4)");
    *fmt = format_of_version(format);
    return kOk;
}

int check_searchable_format(uint8_t format, SplitFormat* fmt) {
    TRY(check_format_byte(format, fmt));
    if (*fmt == kFormatReversible)
        return fail(kInvalidBitstream, "version 4 is the lossless container (quality 100 has no quality to search, and a lossy version 4 is "
                                       "not recommended); use version 3 or 2 for a PSNR floor");
    return kOk;
}

int check_min_psnr(double t) {
    if (std::isnan(t) || t < 0.0) return fail(kInvalidDimensions, "min_psnr_db must be a number >= 0 (or +inf for exact)");
    return kOk;
}

// Buffers of the trials of up to B equal-shaped chunks; one set serves every trial of a call.
struct TrialWork {
    EncodeWork ew;
    DecodeWork dw;
    DevBuf recon, fs;   // one chunk of reconstructed pixels; [B][f] u64 when the caller lends none
    uint32_t B = 0;
    SplitFormat fmt = kFormatSplit;
};

int trial_alloc(TrialWork& t, const ChunkDims& d, uint32_t B, SplitFormat fmt, bool own_frame_sse) {
    t.B = B; t.fmt = fmt;
    const size_t sb = is_wide(fmt) ? 2 : 1;
    t.ew.d = d; t.ew.n_chunks = (int)B;
    t.dw.d = d; t.dw.n_chunks = 1;
    if (transform_tiles_eligible(d)) {
        TRY(t.ew.scratch.alloc(forward_scratch_bytes(d)));
        // one set of buffers serves trials at any step, and the inverse plans its bands by the sample width the step allows
        // (inverse_bounds().mid16): a chunk the i32 plan cuts into bands may stay whole in the i16 plan, whose slot is then
        // the larger of the two.  The slot has to hold either.
        TRY(t.dw.scratch_own.alloc(std::max(inverse_scratch_bytes(d, false), inverse_scratch_bytes(d, true))));
    }
    TRY(t.ew.sym.alloc((size_t)B * 3 * d.padded * sb));
    TRY(t.ew.hist.alloc((size_t)B * 3 * 256 * sizeof(uint32_t)));
    TRY(t.recon.alloc(d.n_pixels * 3));
    if (own_frame_sse) TRY(t.fs.alloc((size_t)B * d.f * sizeof(unsigned long long)));
    return kOk;
}

// n <= t.B chunks at rgb[i], chunk i at q[i]: sse[i] on the host; d_frame_sse (device, [n][f]; null: t.fs) receives the
// per-frame sums.  Returns after the stream has drained.
int trial_run(TrialWork& t, const RgbLayout* rgb, uint32_t n, uint8_t wavelet, const uint8_t* q, hipStream_t st, uint64_t* sse,
              unsigned long long* d_frame_sse) {
    const ChunkDims& d = t.ew.d;
    const bool wide = is_wide(t.fmt);
    const size_t sb = wide ? 2 : 1;
    unsigned long long* fs = d_frame_sse ? d_frame_sse : t.fs.as<unsigned long long>();
    HIP_TRY(hipMemsetAsync(t.ew.hist.p, 0, (size_t)n * 3 * 256 * sizeof(uint32_t), st));
    for (uint32_t i = 0; i < n; ++i)
        TRY(forward_chunk(rgb[i], d, wavelet, quality_to_step(q[i]), t.ew, t.ew.sym.as<uint8_t>() + (size_t)i * 3 * d.padded * sb,
                          t.ew.hist.as<uint32_t>() + (size_t)i * 3 * 256, st, wide));
    const RgbLayout recon = packed_rgb(t.recon.p, d);
    for (uint32_t i = 0; i < n; ++i) {
        const int32_t s = quality_to_step(q[i]);
        const int32_t step[3] = {s, s, s};   // what the encoder writes into the three channel headers
        TRY(inverse_chunk(t.ew.sym.as<uint8_t>() + (size_t)i * 3 * d.padded * sb, d, wavelet, step, t.dw.scratch_own.p, t.dw, recon, st, t.fmt));
        HIP_TRY(launch_rgb_sse(rgb[i], recon, d.w, d.h, d.f, fs + (size_t)i * d.f, st));
    }
    HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> host((size_t)n * d.f);
    TRY(copy_to_host(host.data(), fs, host.size() * sizeof(unsigned long long), st));
    for (uint32_t i = 0; i < n; ++i) {
        uint64_t tot = 0;
        for (uint32_t k = 0; k < d.f; ++k) tot += host[(size_t)i * d.f + k];
        sse[i] = tot;
    }
    return kOk;
}

// floor(65025 N / 10^(T / 10)) in f64; 0 for T = +inf (and wherever the power overflows to it)
uint64_t quality_sse_max(double t, uint64_t n_bytes) {
    const double v = floor(65025.0 * (double)n_bytes / pow(10.0, t / 10.0));
    return v >= 18446744073709551615.0 ? UINT64_MAX : (uint64_t)v;
}

// The rule of alice_codec_encode_to_psnr for one chunk; trial(q, &sse) measures one step.
template <typename Trial>
int quality_choose(uint64_t n_bytes, double min_psnr, uint8_t min_q, uint8_t max_q, Trial trial, uint8_t* chosen, uint8_t* reached,
                   uint64_t* chosen_sse, uint32_t* trials) {
    min_q = std::min<uint8_t>(min_q, 100); max_q = std::min<uint8_t>(max_q, 100);
    const uint64_t sse_max = quality_sse_max(min_psnr, n_bytes);
    uint8_t cand[kQualities];   // coarsest first: the lowest quality of every distinct step in the range
    int n = 0;
    for (int q = min_q; q <= max_q; ++q)
        if (!n || quality_to_step((uint8_t)q) != quality_to_step(cand[n - 1])) cand[n++] = (uint8_t)q;
    *trials = 0;
    auto run = [&](int k, uint64_t* sse) -> int { ++*trials; return trial(cand[k], sse); };
    uint64_t s_fine = 0, s = 0;
    TRY(run(n - 1, &s_fine));
    if (s_fine > sse_max) { *chosen = max_q; *reached = 0; *chosen_sse = s_fine; return kOk; }
    *reached = 1;
    if (n == 1) { *chosen = cand[0]; *chosen_sse = s_fine; return kOk; }
    TRY(run(0, &s));
    if (s <= sse_max) { *chosen = cand[0]; *chosen_sse = s; return kOk; }
    int lo = 0, hi = n - 1;   // lo fails, hi passes
    uint64_t s_hi = s_fine;
    while (hi - lo > 1) {
        const int mid = (lo + hi + 1) / 2;
        TRY(run(mid, &s));
        if (s <= sse_max) { hi = mid; s_hi = s; } else lo = mid;
    }
    *chosen = cand[hi]; *chosen_sse = s_hi;
    return kOk;
}

int quality_choose_chunks(const RgbLayout* rgb, uint32_t n, const ChunkDims& d, uint8_t wavelet, double min_psnr, uint8_t min_q,
                          uint8_t max_q, uint8_t* chosen, uint8_t* reached, double* psnr, hipStream_t st, SplitFormat fmt) {
    tl_quality_trials.assign(n, 0u);
    TrialWork t;
    TRY(trial_alloc(t, d, 1, fmt, true));
    for (uint32_t k = 0; k < n; ++k) {
        uint64_t sse = 0;
        TRY(quality_choose(d.n_pixels * 3, min_psnr, min_q, max_q,
                           [&](uint8_t q, uint64_t* out) -> int { return trial_run(t, rgb + k, 1, wavelet, &q, st, out, nullptr); },
                           chosen + k, reached + k, &sse, &tl_quality_trials[k]));
        psnr[k] = alice_codec_psnr_from_sse(sse, d.n_pixels * 3);
    }
    return kOk;
}

}  // namespace

extern "C" {

double alice_codec_psnr_from_sse(uint64_t sse, uint64_t n_bytes) {
    // the reference sums squared differences in f64; every partial sum is an integer < 2^53, so the
    // integer total converts to the same f64 (src/metrics.rs:26-34)
    if (n_bytes == 0) return INFINITY;  // mse 0.0 for empty buffers (src/metrics.rs:23-25)
    const double mse = (double)sse / (double)n_bytes;
    if (mse == 0.0) return INFINITY;
    return 10.0 * log10(255.0 * 255.0 / mse);
}

int alice_codec_dev_rgb_sse(const void* d_a, uint64_t a_row_pitch, uint64_t a_frame_pitch, const void* d_b, uint64_t b_row_pitch,
                            uint64_t b_frame_pitch, uint32_t width, uint32_t height, uint64_t n_frames, void* d_frame_sse,
                            void* hip_stream) {
    clear_error();
    if (!d_a || !d_b || !d_frame_sse) return fail(kNullArgument, "null argument");
    uint64_t n_pixels = 0;
    TRY(checked_pixel_count(width, height, n_frames, &n_pixels));
    if (n_pixels == 0) return fail(kInvalidDimensions, "invalid dimensions");
    if (n_pixels > UINT64_MAX / 3) return fail(kDimensionOverflow, "dimensions overflow usize");
    const uint64_t row = 3ull * width;
    const uint64_t rp[2] = {a_row_pitch, b_row_pitch}, fp[2] = {a_frame_pitch, b_frame_pitch};
    for (int s = 0; s < 2; ++s) {
        const char* side = s ? "b" : "a";
        if (rp[s] < row) return fail(kInvalidDimensions, std::string("row pitch of ") + side + " is below the " + std::to_string(row) + " bytes of a row");
        const unsigned __int128 span = (unsigned __int128)(height - 1) * rp[s] + row;
        if (fp[s] < span) return fail(kInvalidDimensions, std::string("frame pitch of ") + side + " is below the bytes its rows span");
        if ((unsigned __int128)(n_frames - 1) * fp[s] + span > UINT64_MAX) return fail(kDimensionOverflow, "dimensions overflow usize");
    }
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(launch_rgb_sse(RgbLayout{(uint8_t*)d_a, a_row_pitch, a_frame_pitch}, RgbLayout{(uint8_t*)d_b, b_row_pitch, b_frame_pitch}, width,
                           height, n_frames, (unsigned long long*)d_frame_sse, st));
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}

int alice_codec_dev_trial_sse(uint8_t format, const void* d_frames, uint32_t frame_width, uint32_t frame_height, const uint32_t* origins,
                              uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks, uint8_t wavelet_type, uint8_t quality,
                              const uint8_t* qualities, uint64_t* sse, void* d_frame_sse, void* hip_stream) {
    clear_error();
    if (!d_frames || !sse) return fail(kNullArgument, "null argument");
    SplitFormat fmt;
    TRY(check_format_byte(format, &fmt));
    ChunkDims d{};
    TRY(chunk_dims(width, height, frames, &d, n_chunks));
    std::vector<RgbLayout> layouts;
    TRY(split_layouts(d_frames, frame_width, frame_height, origins, d, n_chunks, layouts));
    if (wavelet_type > 2) return fail(kInvalidBitstream, "unknown wavelet type");
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    std::vector<uint8_t> q(n_chunks);
    for (uint32_t i = 0; i < n_chunks; ++i) q[i] = qualities ? qualities[i] : quality;
    std::vector<uint64_t> out(n_chunks);
    const uint32_t group = split_group(d, fmt);
    TrialWork t;
    TRY(trial_alloc(t, d, std::min(group, n_chunks), fmt, d_frame_sse == nullptr));
    for (uint32_t first = 0; first < n_chunks; first += group) {
        const uint32_t B = std::min(group, n_chunks - first);
        TRY(trial_run(t, layouts.data() + first, B, wavelet_type, q.data() + first, st, out.data() + first,
                      d_frame_sse ? (unsigned long long*)d_frame_sse + (size_t)first * d.f : nullptr));
    }
    for (uint32_t i = 0; i < n_chunks; ++i) sse[i] = out[i];
    return kOk;
}

int alice_codec_dev_encode_to_psnr(uint8_t format, const void* d_frames, uint32_t frame_width, uint32_t frame_height,
                                   const uint32_t* origins, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                   uint8_t wavelet_type, uint32_t lane_symbols, double min_psnr_db, uint8_t min_q, uint8_t max_q,
                                   uint8_t* chosen, uint8_t* reached, double* psnr, void* d_out, uint64_t out_stride, uint64_t* sizes,
                                   void* hip_stream) {
    clear_error();
    if (!d_frames || !chosen || !reached || !psnr || !d_out || !sizes) return fail(kNullArgument, "null argument");
    SplitFormat fmt;
    TRY(check_searchable_format(format, &fmt));
    ChunkDims d{};
    TRY(chunk_dims(width, height, frames, &d, n_chunks));
    std::vector<RgbLayout> layouts;
    TRY(split_layouts(d_frames, frame_width, frame_height, origins, d, n_chunks, layouts));
    uint32_t L = 0;
    TRY(check_split_args(wavelet_type, lane_symbols, &L, fmt));
    TRY(check_quality_range(min_q, max_q));
    TRY(check_min_psnr(min_psnr_db));
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    // the choices reach the caller only with the bytes: a failed call leaves the outputs as they were
    std::vector<uint8_t> q(n_chunks), ok(n_chunks);
    std::vector<double> db(n_chunks);
    std::vector<uint64_t> sz(n_chunks);
    TRY(quality_choose_chunks(layouts.data(), n_chunks, d, wavelet_type, min_psnr_db, min_q, max_q, q.data(), ok.data(), db.data(), st, fmt));
    TRY(split_encode_layouts(layouts.data(), n_chunks, d, wavelet_type, q.data(), L, d_out, out_stride, sz.data(), st, fmt));
    for (uint32_t i = 0; i < n_chunks; ++i) { chosen[i] = q[i]; reached[i] = ok[i]; psnr[i] = db[i]; sizes[i] = sz[i]; }
    return kOk;
}

uint8_t* alice_codec_encode_to_psnr(uint8_t format, uint8_t wavelet_type, const uint8_t* rgb, uint64_t rgb_len, uint32_t width,
                                    uint32_t height, uint32_t frames, uint32_t lane_symbols, double min_psnr_db, uint8_t min_q,
                                    uint8_t max_q, uint8_t* chosen_q, uint8_t* reached, double* psnr, uint64_t* out_len) {
    clear_error();
    if (!chosen_q || !reached || !psnr || !out_len || (!rgb && rgb_len)) { fail(kNullArgument, "null argument"); return nullptr; }
    auto run = [&](uint8_t** out) -> int {
        SplitFormat fmt;
        TRY(check_searchable_format(format, &fmt));
        uint64_t n_pixels = 0;
        TRY(checked_pixel_count(width, height, frames, &n_pixels));
        if (n_pixels == 0 && rgb_len != 0) return fail(kInvalidBufferSize, "buffer size mismatch: expected 0, got " + std::to_string(rgb_len));
        const FrameEncoder enc{0, wavelet_type};
        ChunkDims d{};
        EncodedChunk* none = nullptr;
        if (n_pixels) TRY(validate_encode_many(&enc, rgb, rgb_len, width, height, frames, 1, &none, &d));
        uint32_t L = 0;
        TRY(check_split_args(wavelet_type, lane_symbols, &L, fmt));
        TRY(check_quality_range(min_q, max_q));
        TRY(check_min_psnr(min_psnr_db));
        uint8_t q = 0, ok = 0;
        if (n_pixels == 0) {   // no sample differs at any step
            uint64_t sse = 0;
            tl_quality_trials.assign(1, 0u);
            TRY(quality_choose(0, min_psnr_db, min_q, max_q, [](uint8_t, uint64_t* s) -> int { *s = 0; return kOk; }, &q, &ok, &sse,
                               &tl_quality_trials[0]));
            TRY(host_header_result(kSplitHeaderBytes, out, out_len, [&](uint8_t* p) {
                write_empty_split(p, wavelet_type, width, height, frames, L, quality_to_step(q), format_version(fmt));
            }));
            *chosen_q = q; *reached = ok; *psnr = alice_codec_psnr_from_sse(0, 0);
            return kOk;
        }
        double db = 0.0;
        TRY(host_one_result(rgb, n_pixels * 3, out, out_len, [&](const uint8_t* d_rgb, hipStream_t st, std::vector<uint64_t>& sizes, auto place) -> int {
            const RgbLayout layout = packed_rgb(d_rgb, d);
            TRY(quality_choose_chunks(&layout, 1, d, wavelet_type, min_psnr_db, min_q, max_q, &q, &ok, &db, st, fmt));
            return split_encode_chunks(&layout, 1, d, wavelet_type, &q, L, st, sizes, place, fmt);
        }));
        *chosen_q = q; *reached = ok; *psnr = db;
        return kOk;
    };
    uint8_t* out = nullptr;
    return run(&out) == kOk ? out : nullptr;
}

uint32_t alice_codec_test_last_quality_trials(uint32_t* per_chunk, uint32_t cap) {
    const uint32_t n = (uint32_t)tl_quality_trials.size();
    for (uint32_t i = 0; i < n && i < cap && per_chunk; ++i) per_chunk[i] = tl_quality_trials[i];
    return n;
}

uint64_t alice_codec_test_inverse_scratch_bytes(uint32_t width, uint32_t height, uint32_t frames, int mid16) {
    clear_error();
    ChunkDims d{};
    if (chunk_dims(width, height, frames, &d) != kOk || !transform_tiles_eligible(d)) return 0;
    return inverse_scratch_bytes(d, mid16 != 0);
}

uint64_t alice_codec_test_group_scratch_bytes(uint32_t width, uint32_t height, uint32_t frames, int any16, int any32) {
    clear_error();
    ChunkDims d{};
    if (chunk_dims(width, height, frames, &d) != kOk || !transform_tiles_eligible(d)) return 0;
    return group_scratch_bytes(d, any16 != 0, any32 != 0);
}

void alice_codec_test_set_group_chunks(uint32_t max_chunks) { g_group_chunks_cap.store(max_chunks, std::memory_order_relaxed); }

uint32_t alice_codec_test_group_chunks(uint32_t width, uint32_t height, uint32_t frames, int format) {
    clear_error();
    ChunkDims d{};
    if (format < 2 || format > 4 || chunk_dims(width, height, frames, &d) != kOk) return 0;
    return split_group(d, format_of_version(format));
}

int alice_codec_test_sq_diff_sum(const void* d_a, const void* d_b, uint64_t n, uint64_t* sse, void* hip_stream) {
    clear_error();
    if (!d_a || !d_b || !sse) return fail(kNullArgument, "null argument");
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    DevBuf ds;
    TRY(ds.alloc(8));
    HIP_TRY(hipMemsetAsync(ds.p, 0, 8, st));
    if (n) launch_sq_diff_sum((const uint8_t*)d_a, (const uint8_t*)d_b, n, ds.as<unsigned long long>(), st);
    HIP_TRY(hipGetLastError());
    unsigned long long v = 0;
    TRY(copy_to_host(&v, ds.p, 8, st));
    *sse = v;
    return kOk;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// PART 8: partial decode of a version 2, 3 or 4 chunk, and its first call, the frame range (kernels:
// split_frames_decode_kernel and split_box_decode_kernel of split.hip, the window instances of transform.hip's temporal role)
//
// Every transform is one lifting level per axis and every axis of a channel's [t'][y][x] symbol volume is deinterleaved into
// [low | high], so the positions [c0, c1) of an axis depend on the coefficients of the pairs inside a window [a, b) only
// (axis_window).  A partial call is one plan (the windows, the blocks that hold a kept symbol, where a kept symbol goes), the
// lane stage over the planned blocks (partial_lane_decode) and a finish over the compact volume.  The end checks cover the
// blocks that are read: damage in a lane of another block is not seen.
//
// A frame range is the rectangle of the whole frame: the b - a kept planes, low band then high band, are the symbol volume of
// a virtual chunk of b - a frames whose inverse temporal lifting equals the full chunk's at [t0 - a, t1 - a); the temporal role
// stores t1 - t0 frames and the spatial pass runs over those.
// ------------------------------------------------------------------------------------------

namespace {

uint32_t frames_halo(uint8_t wavelet) { return wavelet == 1 ? 4u : 2u; }   // lifting steps: CDF 9/7 four, CDF 5/3 and Haar two

// the window of an axis of padded length pn and the real positions [c0, c1), c0 < c1 <= pn; ns: frames_halo
void axis_window(uint64_t ns, uint64_t pn, uint64_t c0, uint64_t c1, uint32_t* a, uint32_t* b) {
    *a = c0 > ns ? (uint32_t)((c0 - ns) & ~1ull) : 0u;
    *b = (uint32_t)std::min<uint64_t>(pn, (c1 + ns + 1) & ~1ull);
}

// What a partial call decodes.  The three channels are alike.
struct PartialPlan {
    uint32_t ta = 0, tb = 0, xa = 0, xb = 0, ya = 0, yb = 0;   // the windows
    std::vector<uint32_t> blocks;             // ascending, no duplicates
    bool planes = false;                      // the kept symbols are whole coefficient planes: `ranges`; otherwise `box`
    SplitFramesJob ranges{};                  // a channel's job less its SplitJob; a block both ranges touch belongs to the first
    SplitBoxJob box{};                        // a channel's job less its SplitJob and the list
    uint64_t stored = 0;                      // symbols of a channel that are stored
};

PartialPlan frames_plan(const SplitHeader& h, const ChunkDims& d, uint32_t first, uint32_t count) {
    PartialPlan p;
    axis_window(frames_halo(h.wavelet), d.pf, first, (uint64_t)first + count, &p.ta, &p.tb);
    p.xb = (uint32_t)d.pw; p.yb = (uint32_t)d.ph;
    p.planes = true;
    SplitFramesJob& r = p.ranges;
    const uint64_t P = d.pw * d.ph, half = d.pf / 2, B = 64ull * h.lane_symbols;
    const uint64_t lo0 = p.ta / 2 * P, hi0 = p.tb / 2 * P, lo1 = (half + p.ta / 2) * P, hi1 = (half + p.tb / 2) * P;
    p.stored = (p.tb - p.ta) * P;
    int n_ranges;                             // 1 when the two bands' planes touch (a = 0 and b = pf)
    if (hi0 == lo1) { n_ranges = 1; r.sym_lo[0] = lo0; r.sym_hi[0] = hi1; }
    else { n_ranges = 2; r.sym_lo[0] = lo0; r.sym_hi[0] = hi0; r.sym_lo[1] = lo1; r.sym_hi[1] = hi1; }
    uint64_t next = 0;   // first block no earlier range has taken
    for (int k = 0; k < n_ranges; ++k) {
        const uint64_t f = std::max<uint64_t>(r.sym_lo[k] / B, next), e = (r.sym_hi[k] + B - 1) / B;
        r.blk_first[k] = (uint32_t)f;
        r.blk_count[k] = e > f ? (uint32_t)(e - f) : 0u;
        for (uint64_t blk = f; blk < e; ++blk) p.blocks.push_back((uint32_t)blk);
        next = std::max(next, e);
    }
    return p;
}

// What the calling thread's last call of each kind planned: the test hooks of alice_codec_test.h read their columns
enum PartialKind : int { kPartialFrames = 0, kPartialPreview = 1, kPartialRect = 2 };
struct PartialStats { uint64_t ta, tb, xa, xb, ya, yb, blocks, uploaded, frames, stored; };
thread_local PartialStats tl_partial_stats[3] = {};

// The end of every partial call: the launch status, the drain, and the call's figures
int partial_done(PartialKind kind, const PartialPlan& p, uint32_t count, uint64_t uploaded, hipStream_t st) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    tl_partial_stats[kind] = PartialStats{p.ta, p.tb, p.xa, p.xb, p.ya, p.yb, 3ull * p.blocks.size(), uploaded, count, 3 * p.stored};
    return kOk;
}

// The checks both calls share, in their order (after the null checks): fixed fields and magic, the version byte, that
// version's header checks, then the range.  data: min(len, kSplitHeaderBytes) readable bytes.
// (in two halves, so that a batched call validates a container's header once for all the items that name it)
int frames_validate_header(const uint8_t* data, uint64_t len, SplitHeader& h, ChunkDims& d) {
    if (len < kSplitFixedHeaderBytes)
        return fail(kInvalidBitstream, "data too short for the fixed fields: " + std::to_string(len) + " bytes (they take " +
                                           std::to_string(kSplitFixedHeaderBytes) + ")");
    if (memcmp(data, "ALCC", 4) != 0) return fail(kInvalidBitstream, "bad magic (expected ALCC)");
    const int version = data[4];
    if (version == 1) return fail(kInvalidBitstream, "version 1 has no random access (one serial chain per channel)");
    if (version < 2 || version > 4)
        return fail(kInvalidBitstream, "unsupported version: " + std::to_string(version) + " (a frame range needs version 2, 3 or 4)");
    return parse_split_header(data, len, h, &d, version);
}
int frames_validate_range(const SplitHeader& h, const ChunkDims& d, uint32_t first, uint32_t count) {
    if (count < 1 || (uint64_t)first + count > h.frames)
        return fail(kInvalidDimensions, "frames [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + count) +
                                            ") are not a range of the chunk's " + std::to_string(h.frames) + " frames");
    if (d.n_pixels == 0) return fail(kInvalidDimensions, "invalid dimensions");
    return kOk;
}
int frames_validate(const uint8_t* data, uint64_t len, uint32_t first, uint32_t count, SplitHeader& h, ChunkDims& d) {
    TRY(frames_validate_header(data, len, h, d));
    return frames_validate_range(h, d, first, count);
}

// What the two device calls (frame range, preview) share: the null checks, the header fetched to the host and validated,
// then decode(h, d, stream).  Nothing is queued before the header and the range have been accepted.
template <typename Decode>
int partial_decode_dev(const void* d_alc, uint64_t len, uint32_t first, uint32_t count, const void* d_rgb_out, void* hip_stream, Decode decode) {
    clear_error();
    if (!d_alc || !d_rgb_out) return fail(kNullArgument, "null argument");
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    uint8_t raw[kSplitHeaderBytes] = {};
    if (len) {
        HIP_TRY(hipMemcpyAsync(raw, d_alc, std::min<uint64_t>(len, kSplitHeaderBytes), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    SplitHeader h;
    ChunkDims d{};
    TRY(frames_validate(raw, len, first, count, h, d));
    return decode(h, d, st);
}

// What the two host calls share once h is validated and the blocks are planned (`blocks`: ascending, no duplicates, the
// same for the three channels).  Block offsets come from the tables, on the host; the tables get check_split_directories'
// verdict on the way.  What goes up: the header, the three tables, the byte runs of consecutive planned blocks -- at their
// own offsets of a pool buffer of the container's size, so that the device path runs on it unchanged.  The rest of it
// stays unwritten and unread.  device(d_alc, d_rgb, stream, uploaded payload bytes) decodes `bytes` bytes to d_rgb.
struct PartialSpan { uint64_t off, len; };
// the spans of a container that go up for `blocks`, and the payload bytes among them
int partial_spans(const uint8_t* data, const SplitHeader& h, const std::vector<uint32_t>& blocks, std::vector<PartialSpan>& spans,
                  uint64_t& payload_bytes) {
    spans.push_back({0, kSplitHeaderBytes});
    uint64_t pos = kSplitHeaderBytes;
    payload_bytes = 0;
    for (int c = 0; c < 3; ++c) {
        const uint8_t* tab = data + pos;
        const uint32_t nb = h.n_blocks[c];
        spans.push_back({pos, 4ull * nb});
        uint64_t sum = 4ull * nb;
        size_t next = 0;            // the next planned block
        bool open = false;          // the last span ends where this block starts
        for (uint32_t blk = 0; blk < nb; ++blk) {
            const uint32_t v = get_u32(tab + 4ull * blk);
            if (v < 128u) return fail(kInvalidBitstream, "channel " + std::to_string(c) + ": block " + std::to_string(blk) + " is shorter than its lane directory");
            if (sum + v > h.payload_len[c]) { sum += v; break; }   // (the sum below refuses it; no span may leave the payload)
            if (next < blocks.size() && blocks[next] == blk) {
                if (open) spans.back().len += v; else spans.push_back({pos + sum, v});
                payload_bytes += v;
                open = true;
                ++next;
            } else {
                open = false;
            }
            sum += v;
        }
        if (sum != h.payload_len[c])
            return fail(kInvalidBitstream, "channel " + std::to_string(c) + ": block lengths do not sum to payload_len " + std::to_string(h.payload_len[c]));
        pos += h.payload_len[c];
    }
    return kOk;
}

template <typename Device>
int partial_decode_host(const uint8_t* data, uint64_t len, const SplitHeader& h, const std::vector<uint32_t>& blocks, uint64_t bytes,
                        uint8_t** result, uint64_t* out_len, Device device) {
    std::vector<PartialSpan> spans;
    uint64_t payload_bytes = 0;
    TRY(partial_spans(data, h, blocks, spans, payload_bytes));
    std::unique_ptr<uint8_t, decltype(&free)> out(host_result_alloc(bytes), &free);   // freed on every failure below
    if (!out) return fail(kOutOfMemory, "out of host memory");
    *out_len = bytes;
    hipStream_t st;
    TRY(get_stream(&st));
    DevBuf d_alc, d_rgb;
    TRY(d_alc.alloc(len));
    TRY(d_rgb.alloc(bytes));
    for (const PartialSpan& s : spans)
        HIP_TRY(hipMemcpyAsync(d_alc.as<uint8_t>() + s.off, data + s.off, s.len, hipMemcpyHostToDevice, st));
    TRY(device(d_alc.as<uint8_t>(), d_rgb.p, st, payload_bytes));
    TRY(copy_to_host(out.get(), d_rgb.p, bytes, st));
    *result = out.release();
    return kOk;
}

// The inverse of the virtual chunk dv whose symbols are at d_sym, frames [lo, hi) of it to `rgb` (packed, hi - lo frames):
// inverse_chunk with the window clip.  The instance is the one the full chunk's decode takes (wavelet and steps alone).
int inverse_window(const uint8_t* d_sym, const ChunkDims& dv, uint32_t lo, uint32_t hi, int wavelet, const int32_t step[3], void* d_scratch,
                   DecodeWork& w, const RgbLayout& rgb, hipStream_t st, SplitFormat fmt) {
    const bool wide = is_wide(fmt), mirror = fmt == kFormatReversible;
    const InverseBounds ib = inverse_bounds(wavelet, step, wide ? kWideMaxQ : kByteMaxQ);
    if (d_scratch && launch_inverse_transform_window(d_sym, dv, FrameWindow{lo, hi}, (int)fmt, wavelet, step, ib.exact, ib.mid16, ib.lds16,
                                                     d_scratch, rgb, st))
        return kOk;
    // generic path: the temporal axis over the whole virtual chunk, then the spatial axes, the strip and the colour
    // step over the frames that are kept
    const ChunkDims dx = make_dims(dv.w, dv.h, hi - lo);
    if (!w.planes.p) TRY(w.planes.alloc(3 * dx.n_pixels * sizeof(int16_t)));
    if (!w.tmp.p) TRY(w.tmp.alloc(dv.padded * sizeof(int32_t)));
    if (!w.gen.p) TRY(w.gen.alloc(2 * dv.padded * sizeof(int32_t)));
    int16_t* pl = w.planes.as<int16_t>();
    int32_t* qb = w.gen.as<int32_t>();
    int32_t* vol = qb + dv.padded;
    const uint64_t W = dv.pw, H = dv.ph, D = dv.pf, K = hi - lo;
    int32_t* kept = vol + (size_t)lo * W * H;
    for (int c = 0; c < 3; ++c) {
        if (wide) launch_from_symbols_wide((const uint16_t*)d_sym + (size_t)c * dv.padded, qb, dv.padded, st);
        else launch_from_symbols(d_sym + (size_t)c * dv.padded, qb, dv.padded, st);
        launch_dequantize(qb, vol, dv.padded, step[c], st);
        launch_wavelet_axis(vol, w.tmp.as<int32_t>(), D, W * H, 1, 0, W * H, 1, wavelet, true, st, mirror);
        launch_wavelet_axis(kept, w.tmp.as<int32_t>(), H, W, K, W * H, W, 1, wavelet, true, st, mirror);
        launch_wavelet_axis(kept, w.tmp.as<int32_t>(), W, 1, K * H, W, 1, 0, wavelet, true, st, mirror);
        launch_strip_channel(kept, dx, pl + (size_t)c * dx.n_pixels, st);
    }
    launch_ycocg_to_rgb(pl, pl + dx.n_pixels, pl + 2 * dx.n_pixels, dx, rgb, st);
    return kOk;
}

// The lane stage of a partial call: the planned blocks of the container at d_alc (device, h validated) are decoded and the
// kept symbols of channel c stored in the compact volume at d_sym + c * sym_stride (bytes).  The jobs and the list go up in
// one copy while nothing of the call is queued yet; the verdict of the end checks comes before the caller queues anything
// that writes its output, so a call that is refused for damage in a planned block leaves its output alone, as one that is
// refused by the validation does.  Of the payloads only the block-length tables and the planned blocks are read.
struct LaneStage {
    DevBuf jobs;                 // (before w, as the caller's own buffers are before the LaneStage: w's destructor drains the
    std::vector<uint8_t> up;     //  stream that reads them)
    SplitWork w;
};

int partial_lane_decode(LaneStage& ls, const SplitHeader& h, const ChunkDims& d, const PartialPlan& p, const uint8_t* d_alc, uint8_t* d_sym,
                        size_t sym_stride, hipStream_t st) {
    const bool wide = is_wide(h.fmt);
    const size_t job_bytes = p.planes ? sizeof(SplitFramesJob) : sizeof(SplitBoxJob);
    const size_t list_at = 3 * job_bytes, list_bytes = p.planes ? 0 : p.blocks.size() * sizeof(uint32_t);
    const uint32_t n_planned = (uint32_t)p.blocks.size();
    ls.up.resize(list_at + list_bytes);
    TRY(ls.jobs.alloc(ls.up.size()));
    TRY(split_work_alloc(ls.w, 3, d.padded, h.lane_symbols, false, h.fmt));
    split_chunk_jobs(ls.w, 0, h, d_alc, d_sym, sym_stride);
    for (size_t c = 0; c < 3; ++c) {
        if (p.planes) {
            SplitFramesJob j = p.ranges;
            j.j = ls.w.h[c];
            memcpy(ls.up.data() + c * job_bytes, &j, sizeof(j));
        } else {
            SplitBoxJob j = p.box;
            j.j = ls.w.h[c];
            j.blocks = (const uint32_t*)(ls.jobs.as<uint8_t>() + list_at); j.n_planned = n_planned;
            memcpy(ls.up.data() + c * job_bytes, &j, sizeof(j));
        }
    }
    memcpy(ls.up.data() + list_at, p.blocks.data(), list_bytes);
    ls.w.st = st; ls.w.armed = true;
    HIP_TRY(hipMemcpyAsync(ls.jobs.p, ls.up.data(), ls.up.size(), hipMemcpyHostToDevice, st));
    const std::function<int()> lanes = [&]() -> int {
        if (p.planes) launch_split_frames_decode(ls.jobs.as<SplitFramesJob>(), 3, n_planned, wide, st);
        else launch_split_box_decode(ls.jobs.as<SplitBoxJob>(), 3, n_planned, wide, p.box.n_hi[0] || p.box.n_hi[1], st);
        return kOk;
    };
    TRY(split_decode_launch(ls.w, &h.freq[0][0], st, &lanes));
    return split_decode_verdict(ls.w, st);
}

// The w x rh pixels at (x, y) of frames [first, first + count) of the container at d_alc (device; h, the range and the
// rectangle validated, p their plan) to `out` (device; only the 3 w bytes of each of the rh rows of each frame are written).
// The kept symbols, cut out in axis order, are the symbol volume of a virtual chunk of (xb - xa) x (yb - ya) x (tb - ta)
// whose inverse equals the full chunk's at the rectangle shifted by (xa, ya, ta): the unchanged window inverse runs over it
// and a copy kernel drops the halo.  Returns after the stream has drained.
int rect_decode_device(PartialKind kind, const SplitHeader& h, const ChunkDims& d, const PartialPlan& p, const uint8_t* d_alc, uint32_t first,
                       uint32_t count, uint32_t x, uint32_t y, uint32_t w, uint32_t rh, const RgbLayout& out, hipStream_t st, uint64_t uploaded) {
    const bool wide = is_wide(h.fmt);
    const size_t sb = wide ? 2 : 1;
    // the virtual chunk: even on every axis unless it is the whole frame (no halo to drop), whose pad column and row are the
    // chunk's own
    const bool whole = x == 0 && y == 0 && w == h.width && rh == h.height;
    const ChunkDims dv = make_dims(whole ? h.width : p.xb - p.xa, whole ? h.height : p.yb - p.ya, p.tb - p.ta);
    const ChunkDims dx = make_dims(dv.w, dv.h, count);
    DecodeWork dw;
    dw.d = dv; dw.n_chunks = 1;
    DevBuf d_tmp;
    TRY(dw.sym.alloc(3 * dv.padded * sb));
    if (!whole) TRY(d_tmp.alloc(3 * dx.n_pixels));
    if (transform_tiles_eligible(dv))
        TRY(dw.scratch_own.alloc(inverse_scratch_bytes(dx, inverse_bounds(h.wavelet, h.step, wide ? kWideMaxQ : kByteMaxQ).mid16)));
    LaneStage ls;
    TRY(partial_lane_decode(ls, h, d, p, d_alc, dw.sym.as<uint8_t>(), dv.padded * sb, st));
    const RgbLayout full = whole ? out : packed_rgb(d_tmp.p, dx);
    TRY(inverse_window(dw.sym.as<uint8_t>(), dv, first - p.ta, first - p.ta + count, h.wavelet, h.step, dw.scratch_own.p, dw, full, st, h.fmt));
    if (!whole) launch_rgb_rect_paste(full, x - p.xa, y - p.ya, w, rh, count, out, st);
    return partial_done(kind, p, count, uploaded, st);
}

}  // namespace

extern "C" {

int alice_codec_frames_window(uint8_t wavelet_type, uint32_t frames, uint32_t first, uint32_t count, uint32_t* a, uint32_t* b) {
    clear_error();
    if (!a || !b) return fail(kNullArgument, "null argument");
    if (wavelet_type > 2) return fail(kInvalidBitstream, "unknown wavelet type");
    if (frames == 0xFFFFFFFFu) return fail(kDimensionOverflow, "the padded frame count does not fit 32 bits");
    if (count < 1 || (uint64_t)first + count > frames)
        return fail(kInvalidDimensions, "frames [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + count) +
                                            ") are not a range of the chunk's " + std::to_string(frames) + " frames");
    axis_window(frames_halo(wavelet_type), make_dims(1, 1, frames).pf, first, (uint64_t)first + count, a, b);
    return kOk;
}

int alice_codec_dev_decode_frames(const void* d_alc, uint64_t len, uint32_t first, uint32_t count, void* d_rgb_out, void* hip_stream) {
    return partial_decode_dev(d_alc, len, first, count, d_rgb_out, hip_stream, [&](const SplitHeader& h, const ChunkDims& d, hipStream_t st) {
        return rect_decode_device(kPartialFrames, h, d, frames_plan(h, d, first, count), (const uint8_t*)d_alc, first, count, 0, 0, h.width,
                                  h.height, RgbLayout{(uint8_t*)d_rgb_out, 3ull * h.width, 3ull * h.width * h.height}, st, 0);
    });
}

uint8_t* alice_codec_decode_frames(const uint8_t* data, uint64_t len, uint32_t first, uint32_t count, uint64_t* out_len) {
    clear_error();
    if (!data || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    SplitHeader h;
    ChunkDims d{};
    uint8_t* out = nullptr;
    if (frames_validate(data, len, first, count, h, d) != kOk) return nullptr;
    const PartialPlan p = frames_plan(h, d, first, count);
    partial_decode_host(data, len, h, p.blocks, (uint64_t)h.width * h.height * count * 3, &out, out_len,
                        [&](const uint8_t* d_alc, void* d_rgb, hipStream_t st, uint64_t uploaded) {
                            return rect_decode_device(kPartialFrames, h, d, p, d_alc, first, count, 0, 0, h.width, h.height,
                                                      RgbLayout{(uint8_t*)d_rgb, 3ull * h.width, 3ull * h.width * h.height}, st, uploaded);
                        });
    return out;
}

void alice_codec_test_last_frames_stats(uint64_t out[5]) {
    const PartialStats& s = tl_partial_stats[kPartialFrames];
    const uint64_t v[5] = {s.ta, s.tb, s.blocks, s.uploaded, s.frames};
    if (out) memcpy(out, v, sizeof(v));
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// PART 9: half-resolution preview of a version 2, 3 or 4 chunk from the low band alone (kernels:
// split_box_decode_kernel of split.hip, preview_inv_kernel of transform.hip)
//
// The low-low quadrant [0, ph/2) x [0, pw/2) of every coefficient plane is a half-size picture.  A frame range needs the
// quadrants of its window [a, b) (the temporal lifting runs per (y, x), so the window rule carries over to a sub-rectangle of
// the planes): a box with both runs on t' and the low run alone on x and y.  The top half of a plane is one contiguous symbol
// run, so the blocks of the bottom half are never entropy-decoded, and no spatial inverse runs at all.
// ------------------------------------------------------------------------------------------

namespace {

// the union, over the window's planes t', of the blocks that intersect [t' P, t' P + (qh - 1) pw + qw)
PartialPlan preview_plan(const SplitHeader& h, const ChunkDims& d, uint32_t first, uint32_t count) {
    PartialPlan p;
    axis_window(frames_halo(h.wavelet), d.pf, first, (uint64_t)first + count, &p.ta, &p.tb);
    p.xb = (uint32_t)d.pw; p.yb = (uint32_t)d.ph;
    const uint64_t qw = d.pw / 2, qh = d.ph / 2;
    SplitBoxJob& bx = p.box;
    bx.pw = (uint32_t)d.pw; bx.ph = (uint32_t)d.ph;
    bx.half[0] = (uint32_t)qw; bx.n_lo[0] = (uint32_t)qw;
    bx.half[1] = (uint32_t)qh; bx.n_lo[1] = (uint32_t)qh;
    bx.lo[2] = p.ta / 2; bx.half[2] = (uint32_t)(d.pf / 2); bx.n_lo[2] = bx.n_hi[2] = (p.tb - p.ta) / 2;
    bx.pitch = round_up(qw * qh, 4);          // the plane pitch of the compact volume
    p.stored = (p.tb - p.ta) * qw * qh;
    const uint64_t P = d.pw * d.ph, half = d.pf / 2, B = 64ull * h.lane_symbols, run = (qh - 1) * d.pw + qw;
    for (int band = 0; band < 2; ++band)
        for (uint64_t t = p.ta / 2; t < p.tb / 2; ++t) {
            const uint64_t lo = (band * half + t) * P, hi = lo + run;
            for (uint64_t blk = lo / B; blk <= (hi - 1) / B; ++blk)
                if (p.blocks.empty() || blk > p.blocks.back()) p.blocks.push_back((uint32_t)blk);
        }
    return p;
}

// The preview of frames [first, first + count) of the container at d_alc (device, h validated) to d_rgb (device,
// count * qh * qw * 3 bytes).  Returns after the stream has drained.
int preview_decode_device(const SplitHeader& h, const ChunkDims& d, const PartialPlan& p, const uint8_t* d_alc, uint32_t first,
                          uint32_t count, void* d_rgb, hipStream_t st, uint64_t uploaded) {
    const bool wide = is_wide(h.fmt);
    const size_t sb = wide ? 2 : 1;
    const uint32_t planes = p.tb - p.ta;
    const uint64_t pitch = p.box.pitch, quadrant = (uint64_t)p.box.n_lo[0] * p.box.n_lo[1];
    // the pad symbols of a plane (pitch - qw * qh < 4) are never stored; the finish loads them with a group's real ones
    // and drops what it computes from them, so they need no value
    DevBuf d_sym;
    TRY(d_sym.alloc(3 * (size_t)planes * pitch * sb));
    LaneStage ls;
    TRY(partial_lane_decode(ls, h, d, p, d_alc, d_sym.as<uint8_t>(), (size_t)planes * pitch * sb, st));
    // EXACT is the full chunk's verdict: the first pass inverse_bounds looks at is the temporal one
    const InverseBounds ib = inverse_bounds(h.wavelet, h.step, wide ? kWideMaxQ : kByteMaxQ);
    if (!launch_preview_inverse(d_sym.p, pitch, quadrant, planes, FrameWindow{first - p.ta, first - p.ta + count}, (int)h.fmt, h.wavelet,
                                h.step, ib.exact, (uint8_t*)d_rgb, st))
        return fail(kInternal, "preview: no finish kernel for this volume");
    return partial_done(kPartialPreview, p, count, uploaded, st);
}

}  // namespace

extern "C" {

int alice_codec_preview_dims(uint32_t width, uint32_t height, uint32_t* qw, uint32_t* qh) {
    clear_error();
    if (!qw || !qh) return fail(kNullArgument, "null argument");
    if (width == 0 || height == 0) return fail(kInvalidDimensions, "invalid dimensions");
    *qw = (uint32_t)(((uint64_t)width + 1) / 2);
    *qh = (uint32_t)(((uint64_t)height + 1) / 2);
    return kOk;
}

int alice_codec_dev_decode_preview(const void* d_alc, uint64_t len, uint32_t first, uint32_t count, void* d_rgb_out, void* hip_stream) {
    return partial_decode_dev(d_alc, len, first, count, d_rgb_out, hip_stream, [&](const SplitHeader& h, const ChunkDims& d, hipStream_t st) {
        return preview_decode_device(h, d, preview_plan(h, d, first, count), (const uint8_t*)d_alc, first, count, d_rgb_out, st, 0);
    });
}

uint8_t* alice_codec_decode_preview(const uint8_t* data, uint64_t len, uint32_t first, uint32_t count, uint64_t* out_len) {
    clear_error();
    if (!data || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    SplitHeader h;
    ChunkDims d{};
    if (frames_validate(data, len, first, count, h, d) != kOk) return nullptr;
    const PartialPlan p = preview_plan(h, d, first, count);
    uint8_t* out = nullptr;
    partial_decode_host(data, len, h, p.blocks, (uint64_t)p.box.n_lo[0] * p.box.n_lo[1] * count * 3, &out, out_len,
                        [&](const uint8_t* d_alc, void* d_rgb, hipStream_t st, uint64_t uploaded) {
                            return preview_decode_device(h, d, p, d_alc, first, count, d_rgb, st, uploaded);
                        });
    return out;
}

void alice_codec_test_last_preview_stats(uint64_t out[6]) {
    const PartialStats& s = tl_partial_stats[kPartialPreview];
    const uint64_t v[6] = {s.ta, s.tb, s.blocks, s.uploaded, s.frames, s.stored};
    if (out) memcpy(out, v, sizeof(v));
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// PART 9, batched: many previews in one call (kernels: rans_tables_from_arrays_kernel of rans.hip,
// split_scan_kernel<true> and split_box_decode_kernel<WIDE, false> of split.hip, preview_inv_many_kernel of transform.hip)
//
// A thumbnail strip asks for one frame of each of N chunks, a scrub bar for every k-th frame of one chunk: N times PART 9's
// fixed cost through the single call.  Here the items of a call share one queue: the headers of the distinct containers are
// fetched together, every table of every container is built by one launch, one scan covers every channel, the planned
// blocks of all items are decoded by one lane launch per symbol width (3 jobs per item on blockIdx.y, each with its own
// list), the end checks of all items come back in one copy, and the finish runs once per instance class present.  Every item
// means what PART 9's call means; the call is all or nothing.
// ------------------------------------------------------------------------------------------

namespace {

constexpr uint32_t kPreviewsNoItem = 0xFFFFFFFFu;   // *bad_item of a refusal that is no item's

// What the batched calls share (the previews here, the frame ranges and rectangles of PART 10's batched call): the distinct
// containers, the queue's buffers and counters, and the front of the queue -- headers, tables, scan, the one upload and the
// one verdict.  The lane jobs, the finish and the hook are each call's own.
struct BatchContainer {                    // a distinct (pointer, len) among the items
    const uint8_t* src = nullptr;          // as the caller named it: device memory (dev call) or host memory (host call)
    uint64_t len = 0;
    const uint8_t* d_alc = nullptr;        // on the device
    uint32_t first_item = 0;               // the first item that names it
    uint8_t raw[kSplitHeaderBytes] = {};   // dev call: the header, fetched
    SplitHeader h;
    ChunkDims d{};
    int rc = kOk;                          // the header's verdict, and its message
    std::string msg;
    std::vector<uint32_t> blocks;          // host call: the union of its items' planned blocks
    std::vector<PartialSpan> spans;        // host call: what goes up
};

struct PreviewsItem {
    uint32_t container = 0, first = 0, count = 0;
    PartialPlan p;
    uint8_t* d_rgb = nullptr;
    uint64_t bytes = 0;                    // count * qh * qw * 3
    size_t sym_at = 0;                     // its compact volume inside d_sym
};

// Everything a batched call owns but its items.  settle() drains the stream; the owning struct's destructor calls it
// before any member goes: the host vectors that asynchronous copies read (cs[].raw, up, flags) and the pool buffers
// outlive the work that touches them, also on an error return with kernels still queued.
struct BatchQueue {
    std::vector<BatchContainer> cs;
    std::vector<std::unique_ptr<DevBuf>> alcs;   // host call: one pool buffer of the container's size per distinct container
    DevBuf d_rgb;                                // host call: the outputs, back to back
    DevBuf d_up, d_work, d_sym;
    std::vector<uint8_t> up;
    std::vector<uint32_t> flags;
    hipStream_t st = nullptr;
    bool armed = false;
    uint64_t drains = 0, table_launches = 0, lane_launches = 0, finish_launches = 0;
    void settle() { if (armed) (void)hipStreamSynchronize(st); armed = false; }
    ~BatchQueue() { settle(); }
    int drain() { ++drains; HIP_TRY(hipStreamSynchronize(st)); return kOk; }
};
struct PreviewsBatch : BatchQueue {
    std::vector<PreviewsItem> items;
    ~PreviewsBatch() { settle(); }
};

thread_local uint64_t tl_previews_stats[9] = {};

int fail_item(uint32_t k, uint32_t* bad_item, int code, const std::string& msg) {
    if (bad_item) *bad_item = k;
    return fail(code, "item " + std::to_string(k) + ": " + msg);
}

// The checks that need neither a device nor a byte of a container, then the distinct containers and the items
// (container, first, count, d_rgb of each)
template <typename Item, typename Batch>
int batch_collect(const Item* items, uint32_t n_items, uint32_t max_items, bool dev, uint32_t* bad_item, Batch& b) {
    if (bad_item) *bad_item = kPreviewsNoItem;
    if (!items) return fail(kNullArgument, "null argument");
    if (n_items == 0) return fail(kInvalidDimensions, "a batch holds at least one item");
    if (n_items > max_items)
        return fail(kInvalidDimensions, std::to_string(n_items) + " items: a batch holds at most " + std::to_string(max_items));
    for (uint32_t k = 0; k < n_items; ++k)
        if (!items[k].alc || (dev && !items[k].rgb_out)) return fail_item(k, bad_item, kNullArgument, "null argument");
    std::map<std::pair<const void*, uint64_t>, uint32_t> seen;
    b.items.resize(n_items);
    for (uint32_t k = 0; k < n_items; ++k) {
        const auto at = seen.emplace(std::make_pair(items[k].alc, items[k].len), (uint32_t)b.cs.size());
        if (at.second) {
            b.cs.emplace_back();
            b.cs.back().src = (const uint8_t*)items[k].alc; b.cs.back().len = items[k].len; b.cs.back().first_item = k;
        }
        auto& it = b.items[k];
        it.container = at.first->second; it.first = items[k].first; it.count = items[k].count; it.d_rgb = (uint8_t*)items[k].rgb_out;
    }
    return kOk;
}
int previews_collect(const alice_codec_preview_item* items, uint32_t n_items, bool dev, uint32_t* bad_item, PreviewsBatch& b) {
    return batch_collect(items, n_items, ALICE_PREVIEWS_MAX_ITEMS, dev, bad_item, b);
}

// dev call: every distinct container's header, queued before the first drain
int batch_fetch_headers(BatchQueue& b) {
    b.armed = true;
    bool fetched = false;
    for (BatchContainer& c : b.cs) {
        c.d_alc = c.src;
        if (!c.len) continue;
        HIP_TRY(hipMemcpyAsync(c.raw, c.src, std::min<uint64_t>(c.len, kSplitHeaderBytes), hipMemcpyDeviceToHost, b.st));
        fetched = true;
    }
    if (fetched) TRY(b.drain());
    return kOk;
}

// a container's header is checked once.  header(c): min(len, kSplitHeaderBytes) readable bytes of container c
template <typename Header>
void batch_validate_headers(BatchQueue& b, Header header) {
    for (BatchContainer& c : b.cs) {
        c.rc = frames_validate_header(header(c), c.len, c.h, c.d);
        c.msg = tl_msg;
    }
    clear_error();
}

// frames_validate per item, in item order, with the container's header verdict.  Then every item's plan.
template <typename Header>
int previews_validate(PreviewsBatch& b, uint32_t* bad_item, Header header) {
    batch_validate_headers(b, header);
    for (uint32_t k = 0; k < b.items.size(); ++k) {
        PreviewsItem& it = b.items[k];
        const BatchContainer& c = b.cs[it.container];
        if (c.rc != kOk) return fail_item(k, bad_item, c.rc, c.msg);
        if (frames_validate_range(c.h, c.d, it.first, it.count) != kOk) return fail_item(k, bad_item, tl_err, std::string(tl_msg));
        it.p = preview_plan(c.h, c.d, it.first, it.count);
        it.bytes = (uint64_t)it.p.box.n_lo[0] * it.p.box.n_lo[1] * it.count * 3;
    }
    return kOk;
}

// dev call: no two items' output byte ranges may overlap.  One sort finds whether any do; only a refusal pays for naming
// the first item that overlaps an earlier one.
int previews_outputs_disjoint(const PreviewsBatch& b, uint32_t* bad_item) {
    const size_t n = b.items.size();
    std::vector<std::pair<uintptr_t, uintptr_t>> r(n);
    for (size_t k = 0; k < n; ++k) r[k] = {(uintptr_t)b.items[k].d_rgb, (uintptr_t)b.items[k].d_rgb + b.items[k].bytes};
    std::vector<std::pair<uintptr_t, uintptr_t>> sorted = r;
    std::sort(sorted.begin(), sorted.end());
    bool any = false;
    uintptr_t end = 0;
    for (size_t k = 0; k < n && !any; ++k) {
        any = k > 0 && sorted[k].first < end;
        end = std::max(end, sorted[k].second);
    }
    if (!any) return kOk;
    for (size_t k = 1; k < n; ++k)
        for (size_t j = 0; j < k; ++j)
            if (r[k].first < r[j].second && r[j].first < r[k].second)
                return fail_item((uint32_t)k, bad_item, kInvalidDimensions, "its output overlaps the output of item " + std::to_string(j));
    return fail(kInternal, "previews: overlap not found again");
}

// The front of a batched queue.  What goes up in one copy starts with: frequencies and their prefix sums, the (zero) flags
// (3 per container for the scan, then 3 per item for the lanes), the scan's jobs; the call's own lane jobs, lists and finish
// records follow.  Device scratch: the tables, and every container's block lengths and offsets (per-job block counts:
// containers differ).
inline size_t batch_take(size_t& at, size_t bytes) { const size_t r = at; at = round_up(at + bytes, 256); return r; }
struct BatchFront {
    size_t freq_at = 0, cum_at = 0, flags_at = 0, scan_at = 0, tables_at = 0;
    std::vector<size_t> len_at, off_at;
};
void batch_front_layout(const BatchQueue& b, size_t n_items, size_t& up_n, size_t& work_n, BatchFront& f) {
    const size_t C = b.cs.size();
    f.freq_at = batch_take(up_n, 3 * C * 256 * sizeof(uint16_t)); f.cum_at = batch_take(up_n, 3 * C * 256 * sizeof(uint16_t));
    f.flags_at = batch_take(up_n, (3 * C + 3 * n_items) * sizeof(uint32_t));
    f.scan_at = batch_take(up_n, 3 * C * sizeof(SplitJob));
    f.tables_at = batch_take(work_n, 3 * C * sizeof(RansTable));
    f.len_at.resize(C); f.off_at.resize(C);
    for (size_t i = 0; i < C; ++i) {
        const size_t nb = b.cs[i].h.n_blocks[0];
        f.len_at[i] = batch_take(work_n, 3 * nb * sizeof(uint32_t));
        f.off_at[i] = batch_take(work_n, 3 * (nb + 1) * sizeof(unsigned long long));
    }
}
uint32_t* batch_flags(const BatchQueue& b, const BatchFront& f) { return (uint32_t*)(b.d_up.as<uint8_t>() + f.flags_at); }
// a channel's job less its symbols and its flags (d_up and d_work allocated)
SplitJob batch_channel_job(const BatchQueue& b, const BatchFront& f, size_t ci, int c) {
    const BatchContainer& pc = b.cs[ci];
    const size_t nb = pc.h.n_blocks[0];
    uint8_t* const d_work = b.d_work.as<uint8_t>();
    SplitJob j{};
    uint64_t off = kSplitHeaderBytes;
    for (int e = 0; e < c; ++e) off += pc.h.payload_len[e];
    j.n = pc.d.padded; j.n_blocks = pc.h.n_blocks[c]; j.lane_symbols = pc.h.lane_symbols;
    j.table = (RansTable*)(d_work + f.tables_at) + 3 * ci + (size_t)c;
    j.stream = (uint8_t*)pc.d_alc + off; j.len = pc.h.payload_len[c];
    j.blk_len = (uint32_t*)(d_work + f.len_at[ci]) + (size_t)c * nb;
    j.blk_off = (unsigned long long*)(d_work + f.off_at[ci]) + (size_t)c * (nb + 1);
    return j;
}
// the frequencies, their prefix sums and the scan's jobs into b.up (sized, zeroed)
void batch_front_fill(BatchQueue& b, const BatchFront& f) {
    uint16_t* freq = (uint16_t*)(b.up.data() + f.freq_at);
    uint16_t* cum = (uint16_t*)(b.up.data() + f.cum_at);
    for (size_t ci = 0; ci < b.cs.size(); ++ci)
        for (int c = 0; c < 3; ++c) {
            const size_t t = 3 * ci + (size_t)c;
            uint32_t run = 0;
            for (int i = 0; i < 256; ++i) { freq[t * 256 + i] = b.cs[ci].h.freq[c][i]; cum[t * 256 + i] = (uint16_t)run; run += b.cs[ci].h.freq[c][i]; }
            SplitJob j = batch_channel_job(b, f, ci, c);
            j.flags = batch_flags(b, f) + t;
            memcpy(b.up.data() + f.scan_at + t * sizeof(SplitJob), &j, sizeof(j));
        }
}
// the one upload, every table of every container in one launch, one scan over every channel
int batch_front_launch(BatchQueue& b, const BatchFront& f) {
    const size_t C = b.cs.size();
    uint8_t* const d_up = b.d_up.as<uint8_t>();
    b.armed = true;
    HIP_TRY(hipMemcpyAsync(d_up, b.up.data(), b.up.size(), hipMemcpyHostToDevice, b.st));
    launch_rans_tables_from_arrays((const uint16_t*)(d_up + f.cum_at), (const uint16_t*)(d_up + f.freq_at),
                                   (RansTable*)(b.d_work.as<uint8_t>() + f.tables_at), (int)(3 * C), b.st);
    b.table_launches = 1;
    launch_split_scan((const SplitJob*)(d_up + f.scan_at), (int)(3 * C), true, nullptr, b.st);
    return kOk;
}
// the verdict: every container's and every item's end-check flags in one copy, before anything writes an output
template <typename Batch>
int batch_verdict(Batch& b, const BatchFront& f, uint32_t* bad_item) {
    const size_t C = b.cs.size(), N = b.items.size();
    HIP_TRY(hipGetLastError());
    b.flags.assign(3 * C + 3 * N, 0);
    HIP_TRY(hipMemcpyAsync(b.flags.data(), batch_flags(b, f), b.flags.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, b.st));
    TRY(b.drain());
    for (uint32_t k = 0; k < N; ++k)
        for (int c = 0; c < 3; ++c) {
            const uint32_t scan = b.flags[3 * (size_t)b.items[k].container + (size_t)c], lanes = b.flags[3 * C + 3 * (size_t)k + (size_t)c];
            if ((scan | lanes) & kSplitBadDirectory)
                return fail_item(k, bad_item, kInvalidBitstream, "stream " + std::to_string(c) + ": block or lane directory does not add up");
            if (scan | lanes) return fail_item(k, bad_item, kInvalidBitstream, "stream " + std::to_string(c) + ": a lane failed its end check");
        }
    return kOk;
}

// host call, per distinct container: the union of its items' planned blocks, and the spans that hold them
template <typename Batch>
int batch_host_spans(Batch& b, uint32_t* bad_item, uint64_t& uploaded) {
    for (const auto& it : b.items) {
        std::vector<uint32_t>& u = b.cs[it.container].blocks;
        std::vector<uint32_t> merged;
        std::set_union(u.begin(), u.end(), it.p.blocks.begin(), it.p.blocks.end(), std::back_inserter(merged));
        u.swap(merged);
    }
    uploaded = 0;
    for (BatchContainer& c : b.cs) {
        uint64_t payload = 0;
        if (partial_spans(c.src, c.h, c.blocks, c.spans, payload) != kOk) return fail_item(c.first_item, bad_item, tl_err, std::string(tl_msg));
        uploaded += payload;
    }
    return kOk;
}
// host call: the outputs' buffer, the containers' buffers, and the spans queued
int batch_host_upload(BatchQueue& b, uint64_t total) {
    TRY(b.d_rgb.alloc(total));
    for (BatchContainer& c : b.cs) {
        b.alcs.emplace_back(new DevBuf());
        TRY(b.alcs.back()->alloc(c.len));
        c.d_alc = b.alcs.back()->as<uint8_t>();
    }
    b.armed = true;
    for (const BatchContainer& c : b.cs)
        for (const PartialSpan& s : c.spans)
            HIP_TRY(hipMemcpyAsync((uint8_t*)c.d_alc + s.off, c.src + s.off, s.len, hipMemcpyHostToDevice, b.st));
    return kOk;
}

// The queue of a batched call whose containers are on the device (c.d_alc) and whose items are planned: tables, scan, lanes,
// the verdict of all end checks in one copy, then the finish launches.  Nothing that writes an output is queued before the
// verdict.  drain_at_end: the stream has drained on return (false: the caller's copy to the host drains it).
int previews_device(PreviewsBatch& b, uint32_t* bad_item, bool drain_at_end) {
    hipStream_t st = b.st;
    const size_t C = b.cs.size(), N = b.items.size();
    // after the front: the lane jobs with the narrow items first, their lists, the finish records
    size_t up_n = 0, work_n = 0, sym_n = 0, n_listed = 0;
    std::vector<uint32_t> order;   // lane-job order: items of u8 symbols, then items of u16 symbols
    size_t n_narrow = 0;
    for (int wide = 0; wide < 2; ++wide)
        for (uint32_t k = 0; k < N; ++k)
            if ((int)is_wide(b.cs[b.items[k].container].h.fmt) == wide) { order.push_back(k); if (!wide) ++n_narrow; }
    for (const PreviewsItem& it : b.items) n_listed += it.p.blocks.size();
    BatchFront f;
    batch_front_layout(b, N, up_n, work_n, f);
    const size_t box_at = batch_take(up_n, 3 * N * sizeof(SplitBoxJob));
    const size_t list_at = batch_take(up_n, n_listed * sizeof(uint32_t)), rec_at = batch_take(up_n, N * preview_record_bytes());
    // the pad symbols of a plane (pitch - qw * qh < 4) are never stored; the finish loads them with a group's real ones
    // and drops what it computes from them, so they need no value
    for (PreviewsItem& it : b.items) {
        const size_t sb = is_wide(b.cs[it.container].h.fmt) ? 2 : 1;
        it.sym_at = batch_take(sym_n, 3 * (size_t)(it.p.tb - it.p.ta) * it.p.box.pitch * sb);
    }
    b.up.assign(up_n, 0);
    TRY(b.d_up.alloc(up_n));
    TRY(b.d_work.alloc(work_n));
    TRY(b.d_sym.alloc(sym_n));
    uint8_t* const d_up = b.d_up.as<uint8_t>();
    uint32_t* const d_flags = batch_flags(b, f);
    batch_front_fill(b, f);
    std::vector<PreviewFinish> fin(N);
    uint32_t max_planned[2] = {0, 0};
    size_t listed = 0;
    for (size_t slot = 0; slot < N; ++slot) {
        const uint32_t k = order[slot];
        const PreviewsItem& it = b.items[k];
        const BatchContainer& pc = b.cs[it.container];
        const bool wide = is_wide(pc.h.fmt);
        const size_t sb = wide ? 2 : 1;
        const uint32_t planes = it.p.tb - it.p.ta, n_planned = (uint32_t)it.p.blocks.size();
        uint8_t* const sym = b.d_sym.as<uint8_t>() + it.sym_at;
        memcpy(b.up.data() + list_at + listed * sizeof(uint32_t), it.p.blocks.data(), n_planned * sizeof(uint32_t));
        for (int c = 0; c < 3; ++c) {
            SplitBoxJob j = it.p.box;
            j.j = batch_channel_job(b, f, it.container, c);
            j.j.sym = sym + (size_t)c * planes * it.p.box.pitch * sb;
            j.j.flags = d_flags + 3 * C + 3 * (size_t)k + (size_t)c;
            j.blocks = (const uint32_t*)(d_up + list_at) + listed; j.n_planned = n_planned;
            memcpy(b.up.data() + box_at + (3 * slot + (size_t)c) * sizeof(SplitBoxJob), &j, sizeof(j));
        }
        listed += n_planned;
        max_planned[wide] = std::max(max_planned[wide], n_planned);
        // EXACT is the full chunk's verdict: the first pass inverse_bounds looks at is the temporal one
        PreviewFinish& pf = fin[k];
        pf.d_sym = sym; pf.pitch = it.p.box.pitch; pf.q = (uint64_t)it.p.box.n_lo[0] * it.p.box.n_lo[1]; pf.planes = planes;
        pf.win = FrameWindow{it.first - it.p.ta, it.first - it.p.ta + it.count};
        pf.format = (int)pc.h.fmt; pf.wavelet = pc.h.wavelet;
        for (int c = 0; c < 3; ++c) pf.step[c] = pc.h.step[c];
        pf.exact = inverse_bounds(pc.h.wavelet, pc.h.step, wide ? kWideMaxQ : kByteMaxQ).exact;
        pf.d_rgb = it.d_rgb;
    }
    std::vector<PreviewFinishLaunch> finishes;
    if (!preview_records_plan(fin.data(), (uint32_t)N, b.up.data() + rec_at, finishes))
        return fail(kInternal, "previews: no finish kernel for an item's volume");

    TRY(batch_front_launch(b, f));
    const SplitBoxJob* d_box = (const SplitBoxJob*)(d_up + box_at);
    if (n_narrow) { launch_split_box_decode(d_box, (int)(3 * n_narrow), max_planned[0], false, false, st); ++b.lane_launches; }
    if (N > n_narrow) { launch_split_box_decode(d_box + 3 * n_narrow, (int)(3 * (N - n_narrow)), max_planned[1], true, false, st); ++b.lane_launches; }
    TRY(batch_verdict(b, f, bad_item));
    for (const PreviewFinishLaunch& l : finishes) { launch_preview_inverse_many(d_up + rec_at, l, st); ++b.finish_launches; }
    HIP_TRY(hipGetLastError());
    if (drain_at_end) TRY(b.drain());
    return kOk;
}

void previews_done(const PreviewsBatch& b, uint64_t uploaded) {
    uint64_t blocks = 0, stored = 0;
    for (const PreviewsItem& it : b.items) { blocks += 3ull * it.p.blocks.size(); stored += 3 * it.p.stored; }
    const uint64_t v[9] = {b.items.size(), b.cs.size(), b.table_launches, b.lane_launches, b.finish_launches, b.drains, blocks, uploaded, stored};
    memcpy(tl_previews_stats, v, sizeof(v));
}

}  // namespace

extern "C" {

int alice_codec_dev_decode_previews(const alice_codec_preview_item* items, uint32_t n_items, uint32_t* bad_item, void* hip_stream) {
    clear_error();
    PreviewsBatch b;
    TRY(previews_collect(items, n_items, true, bad_item, b));
    TRY(ensure_device());
    b.st = (hipStream_t)hip_stream;
    ScopeStream scope(b.st);
    TRY(batch_fetch_headers(b));
    TRY(previews_validate(b, bad_item, [](const BatchContainer& c) { return c.raw; }));
    TRY(previews_outputs_disjoint(b, bad_item));
    TRY(previews_device(b, bad_item, true));
    previews_done(b, 0);
    return kOk;
}

uint8_t* alice_codec_decode_previews(const alice_codec_preview_item* items, uint32_t n_items, uint64_t* offsets, uint32_t* bad_item) {
    clear_error();
    PreviewsBatch b;
    if (previews_collect(items, n_items, false, bad_item, b) != kOk) return nullptr;
    if (!offsets) { fail(kNullArgument, "null argument"); return nullptr; }
    if (previews_validate(b, bad_item, [](const BatchContainer& c) { return c.src; }) != kOk) return nullptr;
    uint64_t uploaded = 0, total = 0;
    if (batch_host_spans(b, bad_item, uploaded) != kOk) return nullptr;
    for (const PreviewsItem& it : b.items) total += it.bytes;
    std::unique_ptr<uint8_t, decltype(&free)> out(host_result_alloc(total), &free);   // freed on every failure below
    if (!out) { fail(kOutOfMemory, "out of host memory"); return nullptr; }
    auto run = [&]() -> int {
        TRY(get_stream(&b.st));
        TRY(batch_host_upload(b, total));
        uint64_t at = 0;
        for (PreviewsItem& it : b.items) { it.d_rgb = b.d_rgb.as<uint8_t>() + at; at += it.bytes; }
        TRY(previews_device(b, bad_item, false));
        ++b.drains;
        return copy_to_host(out.get(), b.d_rgb.p, total, b.st);
    };
    if (run() != kOk) return nullptr;
    uint64_t at = 0;
    for (size_t k = 0; k < b.items.size(); ++k) { offsets[k] = at; at += b.items[k].bytes; }
    offsets[b.items.size()] = at;
    previews_done(b, uploaded);
    return out.release();
}

void alice_codec_test_last_previews_stats(uint64_t out[9]) {
    if (out) memcpy(out, tl_previews_stats, sizeof(tl_previews_stats));
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// PART 10: a spatial rectangle of a frame range of a version 2, 3 or 4 chunk (kernels:
// split_box_decode_kernel of split.hip, rgb_rect_paste_kernel of generic.hip)
//
// The window rule holds on x and on y as it holds on t: the pixels of [t0, t1) x [y0, y1) x [x0, x1) depend on the
// coefficients whose coordinate lies, on every axis, in the low or the high run of that axis's window -- a box with both runs
// on every axis.  The body is PART 8's rect_decode_device.
// ------------------------------------------------------------------------------------------

namespace {

// the blocks that intersect an x run of a kept row of a planned plane: planes, rows and runs in ascending position order
PartialPlan rect_plan(const SplitHeader& h, const ChunkDims& d, uint32_t first, uint32_t count, uint32_t x, uint32_t y, uint32_t w, uint32_t rh) {
    PartialPlan p;
    const uint64_t ns = frames_halo(h.wavelet);
    axis_window(ns, d.pf, first, (uint64_t)first + count, &p.ta, &p.tb);
    axis_window(ns, d.pw, x, (uint64_t)x + w, &p.xa, &p.xb);
    axis_window(ns, d.ph, y, (uint64_t)y + rh, &p.ya, &p.yb);
    const uint64_t B = 64ull * h.lane_symbols, hx = d.pw / 2, hy = d.ph / 2, ht = d.pf / 2;
    const bool merged = p.xa == 0 && p.xb == d.pw;
    // both spatial windows are the whole axis: the kept symbols are whole coefficient planes, in plane order (PART 8's plan,
    // whose lane kernel stores with two compares)
    if (merged && p.ya == 0 && p.yb == d.ph) return frames_plan(h, d, first, count);
    p.stored = (uint64_t)(p.tb - p.ta) * (p.yb - p.ya) * (p.xb - p.xa);
    SplitBoxJob& bx = p.box;
    bx.pw = (uint32_t)d.pw; bx.ph = (uint32_t)d.ph;
    bx.lo[0] = p.xa / 2; bx.half[0] = (uint32_t)hx; bx.n_lo[0] = bx.n_hi[0] = (p.xb - p.xa) / 2;
    bx.lo[1] = p.ya / 2; bx.half[1] = (uint32_t)hy; bx.n_lo[1] = bx.n_hi[1] = (p.yb - p.ya) / 2;
    bx.lo[2] = p.ta / 2; bx.half[2] = (uint32_t)ht; bx.n_lo[2] = bx.n_hi[2] = (p.tb - p.ta) / 2;
    bx.pitch = (uint64_t)(p.yb - p.ya) * (p.xb - p.xa);
    // `covered`: where the last listed block ends.  A run that ends at or before it adds nothing, which is what most rows
    // find (a block holds many rows), so the divisions are paid once per new block and not once per row.
    uint64_t covered = 0;
    auto add = [&](uint64_t lo, uint64_t hi) {
        if (hi <= covered) return;
        for (uint64_t blk = std::max(lo, covered) / B; blk <= (hi - 1) / B; ++blk) p.blocks.push_back((uint32_t)blk);
        covered = ((uint64_t)p.blocks.back() + 1) * B;
    };
    const uint64_t rows = (p.yb - p.ya) / 2;
    for (int bt = 0; bt < 2; ++bt)
        for (uint64_t t = bt * ht + p.ta / 2; t < bt * ht + p.tb / 2; ++t)
            for (int by = 0; by < 2; ++by) {
                const uint64_t r0 = by * hy + p.ya / 2;
                if (merged) {   // whole rows: the kept rows of this half of the plane are one run
                    add((t * d.ph + r0) * d.pw, (t * d.ph + r0 + rows) * d.pw);
                    continue;
                }
                for (uint64_t r = r0; r < r0 + rows; ++r) {
                    const uint64_t row = (t * d.ph + r) * d.pw;
                    add(row + p.xa / 2, row + p.xb / 2);
                    add(row + hx + p.xa / 2, row + hx + p.xb / 2);
                }
            }
    return p;
}

// after frames_validate: the rectangle against the frame
int rect_validate(const SplitHeader& h, uint32_t x, uint32_t y, uint32_t w, uint32_t rh) {
    if (w < 1 || rh < 1 || (uint64_t)x + w > h.width || (uint64_t)y + rh > h.height)
        return fail(kInvalidDimensions, "rectangle " + std::to_string(w) + "x" + std::to_string(rh) + " at (" + std::to_string(x) + ", " +
                                            std::to_string(y) + ") does not lie inside the " + std::to_string(h.width) + "x" +
                                            std::to_string(h.height) + " frame");
    return kOk;
}

// the layout of a rectangle's output: packed (both pitches 0), or the caller's pitches, checked
int rect_output_layout(void* d_rgb_out, uint32_t w, uint32_t h, uint64_t row_pitch, uint64_t frame_pitch, RgbLayout& out) {
    out = RgbLayout{(uint8_t*)d_rgb_out, 3ull * w, 3ull * w * h};
    if (row_pitch || frame_pitch) {
        const uint64_t rp = row_pitch ? row_pitch : out.row_pitch;
        const uint64_t fp = frame_pitch ? frame_pitch : rp * h;
        if (rp < 3ull * w || (unsigned __int128)fp < (unsigned __int128)rp * h)
            return fail(kInvalidDimensions, "pitches " + std::to_string(row_pitch) + " and " + std::to_string(frame_pitch) +
                                                " are too small for rows of " + std::to_string(3ull * w) + " bytes and frames of " +
                                                std::to_string(h) + " rows");
        out.row_pitch = rp; out.frame_pitch = fp;
    }
    return kOk;
}

}  // namespace

extern "C" {

int alice_codec_rect_window(uint8_t wavelet_type, uint32_t width, uint32_t height, uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                            uint32_t* xa, uint32_t* xb, uint32_t* ya, uint32_t* yb) {
    clear_error();
    if (!xa || !xb || !ya || !yb) return fail(kNullArgument, "null argument");
    if (wavelet_type > 2) return fail(kInvalidBitstream, "unknown wavelet type");
    if (width == 0xFFFFFFFFu || height == 0xFFFFFFFFu) return fail(kDimensionOverflow, "the padded frame size does not fit 32 bits");
    SplitHeader hd;
    hd.width = width; hd.height = height;
    TRY(rect_validate(hd, x, y, w, h));
    const uint64_t ns = frames_halo(wavelet_type);
    axis_window(ns, (uint64_t)width + (width & 1u), x, (uint64_t)x + w, xa, xb);
    axis_window(ns, (uint64_t)height + (height & 1u), y, (uint64_t)y + h, ya, yb);
    return kOk;
}

int alice_codec_dev_decode_rect(const void* d_alc, uint64_t len, uint32_t first, uint32_t count, uint32_t x, uint32_t y, uint32_t w,
                                uint32_t h, void* d_rgb_out, uint64_t row_pitch, uint64_t frame_pitch, void* hip_stream) {
    return partial_decode_dev(d_alc, len, first, count, d_rgb_out, hip_stream, [&](const SplitHeader& hd, const ChunkDims& d, hipStream_t st) {
        TRY(rect_validate(hd, x, y, w, h));
        RgbLayout out;
        TRY(rect_output_layout(d_rgb_out, w, h, row_pitch, frame_pitch, out));
        return rect_decode_device(kPartialRect, hd, d, rect_plan(hd, d, first, count, x, y, w, h), (const uint8_t*)d_alc, first, count, x, y, w, h,
                                  out, st, 0);
    });
}

uint8_t* alice_codec_decode_rect(const uint8_t* data, uint64_t len, uint32_t first, uint32_t count, uint32_t x, uint32_t y, uint32_t w,
                                 uint32_t h, uint64_t* out_len) {
    clear_error();
    if (!data || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    SplitHeader hd;
    ChunkDims d{};
    if (frames_validate(data, len, first, count, hd, d) != kOk || rect_validate(hd, x, y, w, h) != kOk) return nullptr;
    const PartialPlan p = rect_plan(hd, d, first, count, x, y, w, h);
    uint8_t* out = nullptr;
    partial_decode_host(data, len, hd, p.blocks, 3ull * w * h * count, &out, out_len,
                        [&](const uint8_t* d_alc, void* d_rgb, hipStream_t st, uint64_t uploaded) {
                            return rect_decode_device(kPartialRect, hd, d, p, d_alc, first, count, x, y, w, h,
                                                      RgbLayout{(uint8_t*)d_rgb, 3ull * w, 3ull * w * h}, st, uploaded);
                        });
    return out;
}

void alice_codec_test_last_rect_stats(uint64_t out[10]) {
    const PartialStats& s = tl_partial_stats[kPartialRect];
    const uint64_t v[10] = {s.ta, s.tb, s.xa, s.xb, s.ya, s.yb, s.blocks, s.uploaded, s.frames, s.stored};
    if (out) memcpy(out, v, sizeof(v));
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// PART 10, batched: many frame ranges and rectangles in one call (kernels: rans_tables_from_arrays_kernel
// of rans.hip, split_scan_kernel<true>, split_frames_decode_kernel and split_box_decode_kernel<WIDE, true> of split.hip,
// inv_t_win_many_kernel, inv_t_wide_win_many_kernel and inv_xy_many_kernel of transform.hip, rgb_rect_paste_many_kernel of
// generic.hip)
//
// A detector asks for the same crop of frame k of every chunk, a viewer for a mosaic of crops in one surface: N times PART
// 8's and PART 10's fixed cost through the single calls.  Here the items share the batched preview's queue up to the verdict
// (one table launch, one scan, the lane jobs of all items on blockIdx.y of at most four launches, one copy of all end
// checks) and a finish that runs once per instance class present: the window inverse and the paste over flattened work
// lists.  Every item's virtual chunk, kept-frames slot, compact symbol volume and packed temporary are sub-ranges of pooled
// buffers.  Every item means what the single call means; the call is all or nothing.
// ------------------------------------------------------------------------------------------

namespace {

struct RectsItem {
    uint32_t container = 0, first = 0, count = 0;
    uint32_t x = 0, y = 0, w = 0, h = 0;       // as validated: the whole frame spelled out
    uint64_t row_pitch = 0, frame_pitch = 0;   // as the caller gave them
    PartialPlan p;
    uint8_t* d_rgb = nullptr;
    RgbLayout out{};
    uint64_t bytes = 0;                        // count * h * w * 3
    bool whole = false;                        // the whole frame: the inverse writes the output itself
    bool batched = false;                      // finished by the work-list kernels
    ChunkDims dv{}, dx{};                      // the virtual chunk; its kept frames
    size_t sym_at = 0, slot_at = 0, tmp_at = 0;
    bool has_slot = false;
};

struct RectsBatch : BatchQueue {
    std::vector<RectsItem> items;
    DevBuf d_slot, d_tmp;                               // the band slots; the packed temporaries of the items that paste
    std::vector<std::unique_ptr<DecodeWork>> works;     // per item: the generic path's buffers (null: the item has a band slot)
    uint64_t fallback_items = 0;
    ~RectsBatch() { settle(); }
};

thread_local uint64_t tl_rects_stats[11] = {};

// An output as the disjointness rule sees it
struct RectsOut { uintptr_t base; uint64_t count, h, row_bytes, rp, fp; };
unsigned __int128 rects_out_end(const RectsOut& o) {
    return (unsigned __int128)o.base + (unsigned __int128)(o.count - 1) * o.fp + (unsigned __int128)(o.h - 1) * o.rp + o.row_bytes;
}
// Two outputs conflict when their enclosing byte ranges intersect -- unless both have the same pitches and are disjoint boxes
// of that surface: in coordinates (t, y, x_byte) from the lower base (off = t * fp + y * rp + x_byte, y * rp + x_byte < fp,
// x_byte < rp) each stays a box (x_byte + row_bytes <= rp, (y + h) * rp <= fp), so a byte has one coordinate triple, and the
// boxes are separated on an axis.
bool rects_outputs_conflict(const RectsOut& a, const RectsOut& b) {
    if (!((unsigned __int128)a.base < rects_out_end(b) && (unsigned __int128)b.base < rects_out_end(a))) return false;
    if (a.rp != b.rp || a.fp != b.fp) return true;
    const uintptr_t lower = std::min(a.base, b.base);
    uint64_t t[2], y[2], x[2];
    const RectsOut* o[2] = {&a, &b};
    for (int i = 0; i < 2; ++i) {
        const uint64_t off = o[i]->base - lower, in_frame = off % a.fp;
        t[i] = off / a.fp; y[i] = in_frame / a.rp; x[i] = in_frame % a.rp;
        if (x[i] + o[i]->row_bytes > a.rp || (unsigned __int128)(y[i] + o[i]->h) * a.rp > a.fp) return true;
    }
    const bool apart = t[0] + a.count <= t[1] || t[1] + b.count <= t[0] || y[0] + a.h <= y[1] || y[1] + b.h <= y[0] ||
                       x[0] + a.row_bytes <= x[1] || x[1] + b.row_bytes <= x[0];
    return !apart;
}
// One sweep over the outputs in base order finds whether any two conflict; only a refusal pays for naming the first item, in
// item order, that conflicts with an earlier one.
int rects_outputs_disjoint(const std::vector<RectsOut>& r, uint32_t* bad_item) {
    const size_t n = r.size();
    std::vector<uint32_t> by_base(n), open;
    for (size_t k = 0; k < n; ++k) by_base[k] = (uint32_t)k;
    std::sort(by_base.begin(), by_base.end(), [&](uint32_t a, uint32_t b) { return r[a].base < r[b].base; });
    bool any = false;
    for (size_t i = 0; i < n && !any; ++i) {
        const RectsOut& cur = r[by_base[i]];
        size_t kept = 0;
        for (size_t e = 0; e < open.size(); ++e) {
            if (rects_out_end(r[open[e]]) <= (unsigned __int128)cur.base) continue;   // ends before every later base
            any = any || rects_outputs_conflict(r[open[e]], cur);
            open[kept++] = open[e];
        }
        open.resize(kept);
        open.push_back(by_base[i]);
    }
    if (!any) return kOk;
    for (size_t k = 1; k < n; ++k)
        for (size_t j = 0; j < k; ++j)
            if (rects_outputs_conflict(r[j], r[k]))
                return fail_item((uint32_t)k, bad_item, kInvalidDimensions, "its output overlaps the output of item " + std::to_string(j));
    return fail(kInternal, "rects: overlap not found again");
}

int rects_collect(const alice_codec_rect_item* items, uint32_t n_items, bool dev, uint32_t* bad_item, RectsBatch& b) {
    TRY(batch_collect(items, n_items, ALICE_RECTS_MAX_ITEMS, dev, bad_item, b));
    for (uint32_t k = 0; k < n_items; ++k) {
        RectsItem& it = b.items[k];
        it.x = items[k].x; it.y = items[k].y; it.w = items[k].w; it.h = items[k].h;
        it.row_pitch = dev ? items[k].row_pitch : 0; it.frame_pitch = dev ? items[k].frame_pitch : 0;
    }
    return kOk;
}

// Per item, in item order: frames_validate with the container's header verdict, the rectangle, the pitches.  Then every
// item's plan, as the single call picks it, and its virtual chunk.
template <typename Header>
int rects_validate(RectsBatch& b, uint32_t* bad_item, Header header) {
    batch_validate_headers(b, header);
    for (uint32_t k = 0; k < b.items.size(); ++k) {
        RectsItem& it = b.items[k];
        const BatchContainer& c = b.cs[it.container];
        if (c.rc != kOk) return fail_item(k, bad_item, c.rc, c.msg);
        if (frames_validate_range(c.h, c.d, it.first, it.count) != kOk) return fail_item(k, bad_item, tl_err, std::string(tl_msg));
        const bool range = !it.x && !it.y && !it.w && !it.h;   // a frame range: the whole frame
        if (range) { it.w = c.h.width; it.h = c.h.height; }
        else if (rect_validate(c.h, it.x, it.y, it.w, it.h) != kOk) return fail_item(k, bad_item, tl_err, std::string(tl_msg));
        if (rect_output_layout(it.d_rgb, it.w, it.h, it.row_pitch, it.frame_pitch, it.out) != kOk)
            return fail_item(k, bad_item, tl_err, std::string(tl_msg));
        it.p = range ? frames_plan(c.h, c.d, it.first, it.count) : rect_plan(c.h, c.d, it.first, it.count, it.x, it.y, it.w, it.h);
        it.bytes = 3ull * it.w * it.h * it.count;
        // the virtual chunk, as rect_decode_device derives it
        it.whole = it.x == 0 && it.y == 0 && it.w == c.h.width && it.h == c.h.height;
        it.dv = make_dims(it.whole ? c.h.width : it.p.xb - it.p.xa, it.whole ? c.h.height : it.p.yb - it.p.ya, it.p.tb - it.p.ta);
        it.dx = make_dims(it.dv.w, it.dv.h, it.count);
    }
    return kOk;
}

std::vector<RectsOut> rects_outs(const RectsBatch& b) {
    std::vector<RectsOut> r(b.items.size());
    for (size_t k = 0; k < r.size(); ++k) {
        const RectsItem& it = b.items[k];
        r[k] = RectsOut{(uintptr_t)it.out.base, it.count, it.h, 3ull * it.w, it.out.row_pitch, it.out.frame_pitch};
    }
    return r;
}

// The queue of a batched call whose containers are on the device and whose items are planned (it.out set): the front, at
// most four lane launches, the verdict, the finish.  Nothing that writes an output is queued before the verdict.
int rects_device(RectsBatch& b, uint32_t* bad_item, bool drain_at_end) {
    hipStream_t st = b.st;
    const size_t C = b.cs.size(), N = b.items.size();
    // lane-job order: whole planes before boxes, u8 symbols before u16 symbols in each
    std::vector<uint32_t> order[4];   // [2 * box + wide]
    size_t n_listed = 0, n_batched = 0, n_paste = 0;
    for (uint32_t k = 0; k < N; ++k) {
        RectsItem& it = b.items[k];
        const SplitHeader& h = b.cs[it.container].h;
        order[2 * (it.p.planes ? 0 : 1) + (is_wide(h.fmt) ? 1 : 0)].push_back(k);
        if (!it.p.planes) n_listed += it.p.blocks.size();
        const InverseBounds ib = inverse_bounds(h.wavelet, h.step, is_wide(h.fmt) ? kWideMaxQ : kByteMaxQ);
        it.batched = rects_finish_batchable(it.dv, it.count, ib.exact, ib.mid16);
        if (it.batched) { ++n_batched; if (!it.whole) ++n_paste; }
    }
    const size_t n_frames_jobs = order[0].size() + order[1].size(), n_box_jobs = order[2].size() + order[3].size();
    size_t up_n = 0, work_n = 0, sym_n = 0, slot_n = 0, tmp_n = 0;
    BatchFront f;
    batch_front_layout(b, N, up_n, work_n, f);
    const size_t frames_at = batch_take(up_n, 3 * n_frames_jobs * sizeof(SplitFramesJob));
    const size_t box_at = batch_take(up_n, 3 * n_box_jobs * sizeof(SplitBoxJob));
    const size_t list_at = batch_take(up_n, n_listed * sizeof(uint32_t));
    const size_t t_rec_at = batch_take(up_n, n_batched * rects_record_bytes(0)), xy_rec_at = batch_take(up_n, n_batched * rects_record_bytes(1));
    const size_t paste_rec_at = batch_take(up_n, n_paste * rect_paste_record_bytes());
    for (RectsItem& it : b.items) {
        const SplitHeader& h = b.cs[it.container].h;
        const size_t sb = is_wide(h.fmt) ? 2 : 1;
        it.sym_at = batch_take(sym_n, 3 * it.dv.padded * sb);
        it.has_slot = transform_tiles_eligible(it.dv);
        if (it.has_slot)
            it.slot_at = batch_take(slot_n, inverse_scratch_bytes(it.dx, inverse_bounds(h.wavelet, h.step, is_wide(h.fmt) ? kWideMaxQ : kByteMaxQ).mid16));
        if (!it.whole) it.tmp_at = batch_take(tmp_n, 3 * it.dx.n_pixels);
    }
    b.up.assign(up_n, 0);
    TRY(b.d_up.alloc(up_n));
    TRY(b.d_work.alloc(work_n));
    TRY(b.d_sym.alloc(sym_n));
    TRY(b.d_slot.alloc(slot_n));
    TRY(b.d_tmp.alloc(tmp_n));
    // the generic path's buffers, as inverse_window would allocate them: here, so that no allocation can fail after an
    // output has been written
    for (const RectsItem& it : b.items) {
        b.works.emplace_back(it.has_slot ? nullptr : new DecodeWork());
        if (it.has_slot) continue;
        DecodeWork& dw = *b.works.back();
        dw.d = it.dv; dw.n_chunks = 1;
        TRY(dw.planes.alloc(3 * it.dx.n_pixels * sizeof(int16_t)));
        TRY(dw.tmp.alloc(it.dv.padded * sizeof(int32_t)));
        TRY(dw.gen.alloc(2 * it.dv.padded * sizeof(int32_t)));
    }
    uint8_t* const d_up = b.d_up.as<uint8_t>();
    uint32_t* const d_flags = batch_flags(b, f);
    batch_front_fill(b, f);

    uint32_t max_blocks[4] = {0, 0, 0, 0};
    size_t listed = 0;
    for (int g = 0; g < 4; ++g) {
        const size_t slot0 = (g & 1) ? order[g - 1].size() : 0;   // the wide jobs follow the narrow ones of their kind
        for (size_t s = 0; s < order[g].size(); ++s) {
            const uint32_t k = order[g][s];
            const RectsItem& it = b.items[k];
            const size_t sb = (g & 1) ? 2 : 1, slot = slot0 + s;
            const uint32_t n_planned = (uint32_t)it.p.blocks.size();
            uint8_t* const sym = b.d_sym.as<uint8_t>() + it.sym_at;
            if (g >= 2) memcpy(b.up.data() + list_at + listed * sizeof(uint32_t), it.p.blocks.data(), n_planned * sizeof(uint32_t));
            for (int c = 0; c < 3; ++c) {
                SplitJob sj = batch_channel_job(b, f, it.container, c);
                sj.sym = sym + (size_t)c * it.dv.padded * sb;
                sj.flags = d_flags + 3 * C + 3 * (size_t)k + (size_t)c;
                if (g < 2) {
                    SplitFramesJob j = it.p.ranges;
                    j.j = sj;
                    memcpy(b.up.data() + frames_at + (3 * slot + (size_t)c) * sizeof(SplitFramesJob), &j, sizeof(j));
                } else {
                    SplitBoxJob j = it.p.box;
                    j.j = sj;
                    j.blocks = (const uint32_t*)(d_up + list_at) + listed; j.n_planned = n_planned;
                    memcpy(b.up.data() + box_at + (3 * slot + (size_t)c) * sizeof(SplitBoxJob), &j, sizeof(j));
                }
            }
            if (g >= 2) listed += n_planned;
            max_blocks[g] = std::max(max_blocks[g], n_planned);
        }
    }

    // the finish of the batched items: the window inverse's records, then the pastes'
    std::vector<RectFinish> fin;
    std::vector<RectPaste> pastes;
    for (const RectsItem& it : b.items) {
        if (!it.batched) continue;
        const SplitHeader& h = b.cs[it.container].h;
        const InverseBounds ib = inverse_bounds(h.wavelet, h.step, is_wide(h.fmt) ? kWideMaxQ : kByteMaxQ);
        const RgbLayout full = it.whole ? it.out : packed_rgb(b.d_tmp.as<uint8_t>() + it.tmp_at, it.dx);
        RectFinish r{};
        r.d_sym = b.d_sym.as<uint8_t>() + it.sym_at; r.dv = it.dv;
        r.win = FrameWindow{it.first - it.p.ta, it.first - it.p.ta + it.count};
        r.format = (int)h.fmt; r.wavelet = h.wavelet;
        for (int c = 0; c < 3; ++c) r.step[c] = h.step[c];
        r.exact = ib.exact; r.mid16 = ib.mid16; r.lds16 = ib.lds16;
        r.d_slot = b.d_slot.as<uint8_t>() + it.slot_at; r.rgb = full;
        fin.push_back(r);
        if (!it.whole) pastes.push_back(RectPaste{full, it.x - it.p.xa, it.y - it.p.ya, it.w, it.h, it.count, it.out});
    }
    std::vector<RectFinishLaunch> finishes;
    std::vector<RectPasteLaunch> paste_launches;
    if (!rects_records_plan(fin.data(), (uint32_t)fin.size(), b.up.data() + t_rec_at, b.up.data() + xy_rec_at, finishes) ||
        !rect_paste_records_plan(pastes.data(), (uint32_t)pastes.size(), b.up.data() + paste_rec_at, paste_launches))
        return fail(kInternal, "rects: no finish kernel for an item's volume");

    TRY(batch_front_launch(b, f));
    const SplitFramesJob* d_frames = (const SplitFramesJob*)(d_up + frames_at);
    const SplitBoxJob* d_box = (const SplitBoxJob*)(d_up + box_at);
    if (!order[0].empty()) { launch_split_frames_decode(d_frames, (int)(3 * order[0].size()), max_blocks[0], false, st); ++b.lane_launches; }
    if (!order[1].empty()) { launch_split_frames_decode(d_frames + 3 * order[0].size(), (int)(3 * order[1].size()), max_blocks[1], true, st); ++b.lane_launches; }
    if (!order[2].empty()) { launch_split_box_decode(d_box, (int)(3 * order[2].size()), max_blocks[2], false, true, st); ++b.lane_launches; }
    if (!order[3].empty()) { launch_split_box_decode(d_box + 3 * order[2].size(), (int)(3 * order[3].size()), max_blocks[3], true, true, st); ++b.lane_launches; }
    TRY(batch_verdict(b, f, bad_item));

    for (const RectFinishLaunch& l : finishes) { launch_rects_inverse_many(d_up + t_rec_at, d_up + xy_rec_at, l, st); ++b.finish_launches; }
    for (const RectPasteLaunch& l : paste_launches) { launch_rgb_rect_paste_many(d_up + paste_rec_at, l, st); ++b.finish_launches; }
    // the items the work lists do not take (the generic path; an inverse cut into bands), one after another
    DecodeWork none;   // (an item with a band slot allocates nothing in inverse_window)
    for (size_t k = 0; k < N; ++k) {
        const RectsItem& it = b.items[k];
        if (it.batched) continue;
        const SplitHeader& h = b.cs[it.container].h;
        DecodeWork& dw = b.works[k] ? *b.works[k] : none;
        const RgbLayout full = it.whole ? it.out : packed_rgb(b.d_tmp.as<uint8_t>() + it.tmp_at, it.dx);
        TRY(inverse_window(b.d_sym.as<uint8_t>() + it.sym_at, it.dv, it.first - it.p.ta, it.first - it.p.ta + it.count, h.wavelet, h.step,
                           it.has_slot ? (void*)(b.d_slot.as<uint8_t>() + it.slot_at) : nullptr, dw, full, st, h.fmt));
        if (!it.whole) launch_rgb_rect_paste(full, it.x - it.p.xa, it.y - it.p.ya, it.w, it.h, it.count, it.out, st);
        ++b.fallback_items;
    }
    HIP_TRY(hipGetLastError());
    if (drain_at_end) TRY(b.drain());
    return kOk;
}

void rects_done(const RectsBatch& b, uint64_t uploaded) {
    uint64_t blocks = 0, stored = 0, frames = 0;
    for (const RectsItem& it : b.items) { blocks += 3ull * it.p.blocks.size(); stored += 3 * it.p.stored; frames += it.count; }
    const uint64_t v[11] = {b.items.size(), b.cs.size(), b.table_launches, b.lane_launches, b.finish_launches, b.fallback_items, b.drains,
                            blocks, uploaded, stored, frames};
    memcpy(tl_rects_stats, v, sizeof(v));
}

}  // namespace

extern "C" {

int alice_codec_dev_decode_rects(const alice_codec_rect_item* items, uint32_t n_items, uint32_t* bad_item, void* hip_stream) {
    clear_error();
    RectsBatch b;
    TRY(rects_collect(items, n_items, true, bad_item, b));
    TRY(ensure_device());
    b.st = (hipStream_t)hip_stream;
    ScopeStream scope(b.st);
    TRY(batch_fetch_headers(b));
    TRY(rects_validate(b, bad_item, [](const BatchContainer& c) { return c.raw; }));
    TRY(rects_outputs_disjoint(rects_outs(b), bad_item));
    TRY(rects_device(b, bad_item, true));
    rects_done(b, 0);
    return kOk;
}

uint8_t* alice_codec_decode_rects(const alice_codec_rect_item* items, uint32_t n_items, uint64_t* offsets, uint32_t* bad_item) {
    clear_error();
    RectsBatch b;
    if (rects_collect(items, n_items, false, bad_item, b) != kOk) return nullptr;
    if (!offsets) { fail(kNullArgument, "null argument"); return nullptr; }
    if (rects_validate(b, bad_item, [](const BatchContainer& c) { return c.src; }) != kOk) return nullptr;
    uint64_t uploaded = 0, total = 0;
    if (batch_host_spans(b, bad_item, uploaded) != kOk) return nullptr;
    for (const RectsItem& it : b.items) total += it.bytes;
    std::unique_ptr<uint8_t, decltype(&free)> out(host_result_alloc(total), &free);   // freed on every failure below
    if (!out) { fail(kOutOfMemory, "out of host memory"); return nullptr; }
    auto run = [&]() -> int {
        TRY(get_stream(&b.st));
        TRY(batch_host_upload(b, total));
        uint64_t at = 0;
        for (RectsItem& it : b.items) {
            it.d_rgb = b.d_rgb.as<uint8_t>() + at;
            it.out = RgbLayout{it.d_rgb, 3ull * it.w, 3ull * it.w * it.h};
            at += it.bytes;
        }
        TRY(rects_device(b, bad_item, false));
        ++b.drains;
        return copy_to_host(out.get(), b.d_rgb.p, total, b.st);
    };
    if (run() != kOk) return nullptr;
    uint64_t at = 0;
    for (size_t k = 0; k < b.items.size(); ++k) { offsets[k] = at; at += b.items[k].bytes; }
    offsets[b.items.size()] = at;
    rects_done(b, uploaded);
    return out.release();
}

void alice_codec_test_last_rects_stats(uint64_t out[11]) {
    if (out) memcpy(out, tl_rects_stats, sizeof(tl_rects_stats));
}

int alice_codec_test_rects_outputs_disjoint(const alice_codec_rect_item* items, uint32_t n_items, uint32_t* bad_item) {
    clear_error();
    if (bad_item) *bad_item = kPreviewsNoItem;
    if (!items) return fail(kNullArgument, "null argument");
    std::vector<RectsOut> r(n_items);
    for (uint32_t k = 0; k < n_items; ++k) {
        const alice_codec_rect_item& it = items[k];
        RgbLayout out;
        if (!it.w || !it.h || !it.count) return fail_item(k, bad_item, kInvalidDimensions, "the rule needs an explicit rectangle and a frame count");
        if (rect_output_layout(it.rgb_out, it.w, it.h, it.row_pitch, it.frame_pitch, out) != kOk) return fail_item(k, bad_item, tl_err, std::string(tl_msg));
        r[k] = RectsOut{(uintptr_t)out.base, it.count, it.h, 3ull * it.w, out.row_pitch, out.frame_pitch};
    }
    return rects_outputs_disjoint(r, bad_item);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// PART 11: transcode of version 2, 3 and 4 chunks to a coarser step or a byte budget (kernels:
// transcode.hip)
//
// A symbol is a function of the quantised coefficient alone and the step is stored per channel, so a coarser chunk is made
// from the symbols: lane decode, the map, histogram and table, lane encode.  No transform runs and no pixel exists.  One
// body carries the container (SplitFormat); the lane coders, the table, count and cost kernels are the encoders' own.
// ------------------------------------------------------------------------------------------

namespace {

// The arguments every transcode call shares, after the header has been accepted: lane_symbols (0 keeps the source's),
// then out_version (0 keeps the version; 3 and 4 are interchangeable, only the version byte differs).
int transcode_check_args(const SplitHeader& h, uint32_t lane_symbols, uint8_t out_version, uint32_t* L, SplitFormat* fmt_out) {
    *L = lane_symbols ? lane_symbols : h.lane_symbols;
    if (!split_lane_ok(*L, h.fmt)) return fail(kInvalidDimensions, split_lane_msg(h.fmt));
    const bool ok = out_version == 0 || (is_wide(h.fmt) && (out_version == 3 || out_version == 4));
    if (!ok)
        return fail(kInvalidDimensions, "out_version " + std::to_string((int)out_version) + " of a version " + std::to_string((int)format_version(h.fmt)) +
                                            " chunk (0 keeps the version; 3 and 4 for a version 3 or 4 chunk)");
    *fmt_out = out_version ? format_of_version(out_version) : h.fmt;
    return kOk;
}

int transcode_check_budget_format(SplitFormat fmt_out) {
    if (fmt_out == kFormatReversible)
        return fail(kInvalidBitstream, "version 4 is the lossless container (a byte budget searches the quality, and a lossy version 4 is "
                                       "not recommended); ask for out_version = 3");
    return kOk;
}

// step and dead zone channel c of a chunk gets at target step s2: untouched unless the target is coarser
inline void transcode_channel_steps(const SplitHeader& h, int c, int32_t s2, int32_t* step, int32_t* dead_zone) {
    const bool coarser = s2 > h.step[c];
    *step = coarser ? s2 : h.step[c];
    *dead_zone = coarser ? s2 : h.dead_zone[c];
}

// The decoded symbols of B equal-shaped chunks of one version, resident for the whole call: chunk i, channel c at
// sym + (3 i + c) * padded * sb.
struct TranscodeSource {
    DevBuf sym;
    SplitWork dw;
    size_t sb = 1;
};

// Queues the directory scan and the lane decode of the chunks at d_alc[i] (hdr[i] validated) and returns with their verdict:
// nothing of a damaged source is mapped or written.
int transcode_decode(TranscodeSource& s, const SplitHeader* hdr, const uint8_t* const* d_alc, uint32_t B, const ChunkDims& d, hipStream_t st) {
    const SplitFormat fmt = hdr[0].fmt;
    s.sb = is_wide(fmt) ? 2 : 1;
    TRY(s.sym.alloc((size_t)B * 3 * d.padded * s.sb));
    TRY(split_work_alloc(s.dw, (int)(3 * B), d.padded, hdr[0].lane_symbols, false, fmt));
    std::vector<uint16_t> freq((size_t)B * 3 * 256);
    for (uint32_t i = 0; i < B; ++i) {
        split_chunk_jobs(s.dw, 3 * (size_t)i, hdr[i], d_alc[i], s.sym.as<uint8_t>() + 3 * (size_t)i * d.padded * s.sb, d.padded * s.sb);
        memcpy(&freq[3 * (size_t)i * 256], hdr[i].freq, 3 * 256 * sizeof(uint16_t));
    }
    TRY(split_decode_launch(s.dw, freq.data(), st));
    return split_decode_verdict(s.dw, st);
}

// The first half of an encode from symbols: B chunks whose source symbols lie at `in` (chunk stride 3 * padded * sb) are
// mapped to target step s2[i] into `out` (in == out: in place, untouched channels are only counted), then the tables and
// the count pass.  Returns the exact container sizes after the stream has drained; split_write_chunks(e, ...) writes them.
int transcode_count_chunks(SplitChunkEncode& e, const uint8_t* in, uint8_t* out, const SplitHeader* hdr, uint32_t B, const ChunkDims& d,
                           const int32_t* s2, uint32_t L, SplitFormat fmt_out, hipStream_t st, std::vector<uint64_t>& sizes) {
    const bool wide = is_wide(fmt_out);
    const size_t sb = wide ? 2 : 1;
    e.B = B; e.L = L; e.wavelet = hdr[0].wavelet; e.fmt = fmt_out;
    e.q.assign(B, 0);
    e.steps.assign(3 * (size_t)B, 1); e.dead_zones.assign(3 * (size_t)B, 1);
    e.ew.d = d; e.ew.n_chunks = (int)B;
    TRY(e.ew.hist.alloc((size_t)B * 3 * 256 * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(e.ew.hist.p, 0, (size_t)B * 3 * 256 * sizeof(uint32_t), st));
    for (uint32_t i = 0; i < B; ++i)
        for (int c = 0; c < 3; ++c) {
            const size_t j = 3 * (size_t)i + c;
            transcode_channel_steps(hdr[i], c, s2[i], &e.steps[j], &e.dead_zones[j]);
            const uint8_t* src = in + j * d.padded * sb;
            uint8_t* dst = out + j * d.padded * sb;
            uint32_t* hist = e.ew.hist.as<uint32_t>() + j * 256;
            if (src != dst || s2[i] > hdr[i].step[c]) launch_requant_symbols(src, dst, d.padded, wide, hdr[i].step[c], s2[i], hist, st);
            else if (wide) launch_histogram_wide((const uint16_t*)src, d.padded, hist, st);
            else launch_histogram(src, d.padded, hist, st);
        }
    HIP_TRY(hipGetLastError());
    e.hd.assign(B, SplitHeaderDesc{});
    TRY(split_work_alloc(e.w, (int)(3 * B), d.padded, L, true, fmt_out));
    for (size_t j = 0; j < 3 * (size_t)B; ++j) e.w.h[j].sym = out + j * d.padded * sb;
    TRY(split_count(e.w, e.ew.hist.as<uint32_t>(), st, e.totals, nullptr));
    sizes.resize(B);
    for (uint32_t i = 0; i < B; ++i) sizes[i] = kSplitHeaderBytes + e.totals[3 * i] + e.totals[3 * i + 1] + e.totals[3 * i + 2];
    return kOk;
}

// Payload brackets of B resident chunks at every target step: out[(chunk * 64 + step - 1) * 3 + channel], as predict_chunks
// gives them for an encode.  The bins are of the value the map quantises (launch_symbol_bins), folded by the encoders' fold;
// the rows of steps at or below a channel's own step are its own coded histogram (the channel is left untouched there).  A
// chunk with values outside the bins' range gets its rows from real maps at each coarser step.  Returns after the stream
// has drained.
int transcode_predict_chunks(const TranscodeSource& s, const SplitHeader* hdr, uint32_t B, const ChunkDims& d, uint32_t L, hipStream_t st,
                             std::vector<RateChannel>& out) {
    const bool wide = is_wide(hdr[0].fmt);
    const size_t per_chunk = (size_t)64 * 3;
    DevBuf bins, oor, src_hist, step_hist, res, logt, scratch;
    StreamDrain drain(st);
    TRY(bins.alloc((size_t)B * 3 * 4096 * sizeof(uint32_t)));
    TRY(oor.alloc((size_t)B * sizeof(uint32_t)));
    TRY(src_hist.alloc((size_t)B * 3 * 256 * sizeof(uint32_t)));
    TRY(step_hist.alloc((size_t)B * per_chunk * 256 * sizeof(uint32_t)));
    TRY(res.alloc((size_t)B * per_chunk * sizeof(RateChannel)));
    TRY(logt.alloc(2 * (kProbScale + 1) * sizeof(uint32_t)));
    const RateLogTable& t = rate_log_table();
    HIP_TRY(hipMemcpyAsync(logt.p, t.lo, sizeof(t.lo), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(logt.as<uint32_t>() + (kProbScale + 1), t.hi, sizeof(t.hi), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(bins.p, 0, (size_t)B * 3 * 4096 * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(oor.p, 0, (size_t)B * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(src_hist.p, 0, (size_t)B * 3 * 256 * sizeof(uint32_t), st));
    auto sym_of = [&](uint32_t i, int c) { return s.sym.as<uint8_t>() + (3 * (size_t)i + c) * d.padded * s.sb; };
    for (uint32_t i = 0; i < B; ++i)
        for (int c = 0; c < 3; ++c) {
            launch_symbol_bins(sym_of(i, c), d.padded, wide, hdr[i].step[c], bins.as<uint32_t>() + (3 * (size_t)i + c) * 4096, oor.as<uint32_t>() + i, st);
            uint32_t* h = src_hist.as<uint32_t>() + (3 * (size_t)i + c) * 256;
            if (wide) launch_histogram_wide((const uint16_t*)sym_of(i, c), d.padded, h, st);
            else launch_histogram(sym_of(i, c), d.padded, h, st);
        }
    if (wide) launch_rate_fold_wide(bins.as<uint32_t>(), oor.as<uint32_t>(), B, step_hist.as<uint32_t>(), st);
    else launch_rate_fold(bins.as<uint32_t>(), oor.as<uint32_t>(), B, step_hist.as<uint32_t>(), st);
    std::vector<uint32_t> h_oor(B);
    HIP_TRY(hipMemcpyAsync(h_oor.data(), oor.p, B * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < B; ++i) {
        uint32_t* rows = step_hist.as<uint32_t>() + (size_t)i * per_chunk * 256;
        if (h_oor[i]) {
            if (!scratch.p) TRY(scratch.alloc(d.padded * s.sb));
            HIP_TRY(hipMemsetAsync(rows, 0, per_chunk * 256 * sizeof(uint32_t), st));
            for (int c = 0; c < 3; ++c)
                for (int32_t step = hdr[i].step[c] + 1; step <= 64; ++step)
                    launch_requant_symbols(sym_of(i, c), scratch.p, d.padded, wide, hdr[i].step[c], step, rows + ((size_t)(step - 1) * 3 + c) * 256, st);
        }
        launch_kept_rows(src_hist.as<uint32_t>() + 3 * (size_t)i * 256, hdr[i].step, rows, st);
    }
    if (wide) launch_wide_rate_cost(step_hist.as<uint32_t>(), logt.as<uint32_t>(), B, L, res.as<RateChannel>(), st);
    else launch_split_rate_cost(step_hist.as<uint32_t>(), logt.as<uint32_t>(), B, L, res.as<RateChannel>(), st);
    HIP_TRY(hipGetLastError());
    out.resize((size_t)B * per_chunk);
    HIP_TRY(hipMemcpyAsync(out.data(), res.p, out.size() * sizeof(RateChannel), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}

// The qualities of the B resident chunks under their budgets: split_choose_quality unchanged.  A trial maps the chunk's
// resident symbols into a scratch copy, then the table and the count pass; nothing is decoded again.
int transcode_choose_chunks(const TranscodeSource& s, const SplitHeader* hdr, uint32_t B, const ChunkDims& d, uint32_t L, SplitFormat fmt_out,
                            const uint64_t* budgets, uint8_t min_q, uint8_t max_q, uint8_t* chosen, uint8_t* fits, uint32_t* trials, hipStream_t st) {
    std::vector<RateChannel> rc;
    TRY(transcode_predict_chunks(s, hdr, B, d, L, st, rc));
    DevBuf scratch;
    StreamDrain drain(st);
    uint64_t lo[kQualities], hi[kQualities];
    for (uint32_t i = 0; i < B; ++i) {
        split_rate_by_quality(rc.data() + (size_t)i * 192, lo, hi);
        TRY(split_choose_quality(lo, hi, budgets[i], min_q, max_q,
                                 [&](uint8_t q, uint64_t* size) -> int {
                                     if (!scratch.p) TRY(scratch.alloc(3 * d.padded * s.sb));
                                     SplitChunkEncode e;
                                     std::vector<uint64_t> sz;
                                     const int32_t s2 = quality_to_step(q);
                                     TRY(transcode_count_chunks(e, s.sym.as<uint8_t>() + 3 * (size_t)i * d.padded * s.sb, scratch.as<uint8_t>(), hdr + i, 1, d,
                                                                &s2, L, fmt_out, st, sz));
                                     *size = sz[0];
                                     return kOk;
                                 },
                                 chosen + i, fits + i, trials + i));
    }
    return kOk;
}

// One group of a transcode: decode, (budgets: choose the qualities,) map in place and count, place(sizes, outs), write.
// q: the target quality per chunk; with budgets it is written (and fits) before the map.
template <typename Place>
int transcode_group(const SplitHeader* hdr, const uint8_t* const* d_alc, uint32_t B, const ChunkDims& d, uint8_t* q, uint32_t L,
                    SplitFormat fmt_out, const uint64_t* budgets, uint8_t min_q, uint8_t max_q, uint8_t* fits, uint32_t* trials,
                    hipStream_t st, std::vector<uint64_t>& sizes, Place place) {
    TranscodeSource s;
    SplitChunkEncode e;     // (after s: its destructor drains the stream that reads s.sym)
    TRY(transcode_decode(s, hdr, d_alc, B, d, st));
    if (budgets) TRY(transcode_choose_chunks(s, hdr, B, d, L, fmt_out, budgets, min_q, max_q, q, fits, trials, st));
    std::vector<int32_t> s2(B);
    for (uint32_t i = 0; i < B; ++i) s2[i] = quality_to_step(q[i]);
    TRY(transcode_count_chunks(e, s.sym.as<uint8_t>(), s.sym.as<uint8_t>(), hdr, B, d, s2.data(), L, fmt_out, st, sizes));
    std::vector<uint8_t*> outs(B, nullptr);
    TRY(place(sizes, outs));
    return split_write_chunks(e, outs, st);
}

// A chunk without pixels is its header: the steps, lane_symbols and the version byte change in place.
void transcode_empty(uint8_t* p, const SplitHeader& h, int32_t s2, uint32_t L, SplitFormat fmt_out) {
    p[4] = format_version(fmt_out);
    put_u32(p + 18, L);
    for (int c = 0; c < 3; ++c) {
        int32_t step, dz;
        transcode_channel_steps(h, c, s2, &step, &dz);
        uint8_t* qh = p + kSplitFixedHeaderBytes + (size_t)c * kSplitChannelHeaderBytes;
        put_u32(qh, (uint32_t)step); put_u32(qh + 4, (uint32_t)dz);
    }
}

// The host calls: data validated on the host (header, arguments, directories) before a device is looked for.
uint8_t* transcode_host(const uint8_t* data, uint64_t len, uint8_t quality, uint32_t lane_symbols, uint8_t out_version, const uint64_t* max_bytes,
                        uint8_t min_q, uint8_t max_q, uint8_t* chosen_q, uint8_t* fits, uint64_t* out_len) {
    auto run = [&](uint8_t** out) -> int {
        SplitHeader h;
        ChunkDims d{};
        TRY(frames_validate_header(data, len, h, d));
        uint32_t L = 0;
        SplitFormat fmt_out;
        TRY(transcode_check_args(h, lane_symbols, out_version, &L, &fmt_out));
        if (max_bytes) {
            TRY(check_quality_range(min_q, max_q));
            TRY(transcode_check_budget_format(fmt_out));
        }
        TRY(check_split_directories(data, h));
        uint8_t q = quality, ok = 1;
        uint32_t trials = 0;
        if (d.n_pixels == 0) {
            if (max_bytes) {
                uint64_t lo[kQualities], hi[kQualities];
                for (int k = 0; k < kQualities; ++k) lo[k] = hi[k] = kSplitHeaderBytes;
                TRY(split_choose_quality(lo, hi, *max_bytes, min_q, max_q, [](uint8_t, uint64_t*) -> int { return kOk; }, &q, &ok, &trials));
                tl_split_trials.assign(1, trials);
            }
            TRY(host_header_result(kSplitHeaderBytes, out, out_len, [&](uint8_t* p) {
                memcpy(p, data, kSplitHeaderBytes);
                transcode_empty(p, h, quality_to_step(q), L, fmt_out);
            }));
        } else {
            TRY(host_one_result(data, len, out, out_len, [&](const uint8_t* d_alc, hipStream_t st, std::vector<uint64_t>& sizes, auto place) -> int {
                TRY(transcode_group(&h, &d_alc, 1, d, &q, L, fmt_out, max_bytes, min_q, max_q, &ok, &trials, st, sizes, place));
                if (max_bytes) tl_split_trials.assign(1, trials);   // (the trials of a group that ran, whatever becomes of the download)
                return kOk;
            }));
        }
        if (max_bytes) { *chosen_q = q; *fits = ok; }
        return kOk;
    };
    uint8_t* out = nullptr;
    return run(&out) == kOk ? out : nullptr;
}

// The headers of n device containers of any of the versions 2 to 4 (the transcodes, the repack to version 5): the chunks
// agree in version, wavelet, shape and lane_symbols.
int source_device_headers(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks, hipStream_t st,
                          std::vector<SplitHeader>& hdr, std::vector<const uint8_t*>& ptr, ChunkDims& d) {
    return read_device_headers(d_alc, alc_stride, sizes, n_chunks, kSplitHeaderBytes, st, frames_validate_header,
                               [](const SplitHeader& h0, const SplitHeader& hi) {
                                   return hi.fmt == h0.fmt && hi.wavelet == h0.wavelet && hi.lane_symbols == h0.lane_symbols;
                               },
                               "the chunks of one call must have the same version, wavelet, shape and lane_symbols", hdr, ptr, d);
}

// The device calls: the headers come to the host first, and nothing is queued before they and the arguments have been
// accepted.  budgets == NULL: chunk i at q[i].
int transcode_device(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks, uint8_t* q, uint32_t lane_symbols,
                     uint8_t out_version, const uint64_t* budgets, uint8_t min_q, uint8_t max_q, uint8_t* fits, void* d_out,
                     uint64_t out_stride, uint64_t* out_sizes, hipStream_t st) {
    std::vector<SplitHeader> hdr;
    std::vector<const uint8_t*> ptr;
    ChunkDims d{};
    TRY(source_device_headers(d_alc, alc_stride, sizes, n_chunks, st, hdr, ptr, d));
    uint32_t L = 0;
    SplitFormat fmt_out;
    TRY(transcode_check_args(hdr[0], lane_symbols, out_version, &L, &fmt_out));
    if (budgets) TRY(transcode_check_budget_format(fmt_out));
    std::vector<uint32_t> trials(n_chunks, 0u);
    TRY(for_each_group(n_chunks, split_group(d, hdr[0].fmt), out_sizes, [&](uint32_t first, uint32_t B, std::vector<uint64_t>& sz) {
        return transcode_group(hdr.data() + first, ptr.data() + first, B, d, q + first, L, fmt_out, budgets ? budgets + first : nullptr, min_q, max_q,
                               fits ? fits + first : nullptr, trials.data() + first, st, sz, place_strided(d_out, out_stride, first, B));
    }));
    if (budgets) tl_split_trials = trials;
    return kOk;
}

}  // namespace

extern "C" {

uint8_t* alice_codec_transcode(const uint8_t* data, uint64_t len, uint8_t quality, uint32_t lane_symbols, uint8_t out_version, uint64_t* out_len) {
    clear_error();
    if (!data || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    return transcode_host(data, len, quality, lane_symbols, out_version, nullptr, 0, 0, nullptr, nullptr, out_len);
}

uint8_t* alice_codec_transcode_to_size(const uint8_t* data, uint64_t len, uint32_t lane_symbols, uint8_t out_version, uint64_t max_bytes,
                                       uint8_t min_q, uint8_t max_q, uint8_t* chosen_q, uint8_t* fits, uint64_t* out_len) {
    clear_error();
    if (!data || !chosen_q || !fits || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    return transcode_host(data, len, 0, lane_symbols, out_version, &max_bytes, min_q, max_q, chosen_q, fits, out_len);
}

int alice_codec_predict_transcode_sizes(const uint8_t* data, uint64_t len, uint32_t lane_symbols, uint64_t lo[101], uint64_t hi[101]) {
    clear_error();
    if (!data || !lo || !hi) return fail(kNullArgument, "null argument");
    SplitHeader h;
    ChunkDims d{};
    TRY(frames_validate_header(data, len, h, d));
    uint32_t L = 0;
    SplitFormat fmt_out;
    TRY(transcode_check_args(h, lane_symbols, 0, &L, &fmt_out));
    TRY(check_split_directories(data, h));
    if (d.n_pixels == 0) {   // an empty chunk is its header at every quality
        for (int q = 0; q < kQualities; ++q) lo[q] = hi[q] = kSplitHeaderBytes;
        return kOk;
    }
    hipStream_t st;
    TRY(get_stream(&st));
    DevBuf d_alc;
    TranscodeSource s;
    StreamDrain drain(st);
    TRY(d_alc.alloc(len));
    HIP_TRY(hipMemcpyAsync(d_alc.p, data, len, hipMemcpyHostToDevice, st));
    const uint8_t* p = d_alc.as<uint8_t>();
    TRY(transcode_decode(s, &h, &p, 1, d, st));
    std::vector<RateChannel> rc;
    TRY(transcode_predict_chunks(s, &h, 1, d, L, st, rc));
    split_rate_by_quality(rc.data(), lo, hi);
    return kOk;
}

int alice_codec_dev_transcode(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks, uint8_t quality,
                              const uint8_t* qualities, uint32_t lane_symbols, uint8_t out_version, void* d_out, uint64_t out_stride,
                              uint64_t* out_sizes, void* hip_stream) {
    clear_error();
    if (!d_out || !out_sizes) return fail(kNullArgument, "null argument");
    TRY(check_dev_containers(d_alc, alc_stride, sizes, n_chunks));
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    std::vector<uint8_t> q(n_chunks);
    for (uint32_t i = 0; i < n_chunks; ++i) q[i] = qualities ? qualities[i] : quality;
    return transcode_device(d_alc, alc_stride, sizes, n_chunks, q.data(), lane_symbols, out_version, nullptr, 0, 0, nullptr, d_out, out_stride,
                            out_sizes, st);
}

int alice_codec_dev_transcode_to_budget(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks, uint32_t lane_symbols,
                                        uint8_t out_version, const uint64_t* budgets, uint8_t min_q, uint8_t max_q, uint8_t* chosen,
                                        uint8_t* fits, void* d_out, uint64_t out_stride, uint64_t* out_sizes, void* hip_stream) {
    clear_error();
    if (!d_out || !out_sizes) return fail(kNullArgument, "null argument");
    TRY(check_dev_containers(d_alc, alc_stride, sizes, n_chunks));
    if (!budgets || !chosen || !fits) return fail(kNullArgument, "null argument");
    TRY(check_quality_range(min_q, max_q));
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    // the choices reach the caller only with the bytes: a failed call leaves chosen / fits / out_sizes as they were
    std::vector<uint8_t> q(n_chunks), ok(n_chunks);
    std::vector<uint64_t> sz(n_chunks);
    TRY(transcode_device(d_alc, alc_stride, sizes, n_chunks, q.data(), lane_symbols, out_version, budgets, min_q, max_q, ok.data(), d_out,
                         out_stride, sz.data(), st));
    for (uint32_t i = 0; i < n_chunks; ++i) { chosen[i] = q[i]; fits[i] = ok[i]; out_sizes[i] = sz[i]; }
    return kOk;
}

int alice_codec_dev_requant_symbols(const void* d_src, void* d_dst, uint64_t n, int wide, int32_t step_from, int32_t step_to, void* d_hist,
                                    void* hip_stream) {
    clear_error();
    if ((!d_src || !d_dst) && n) return fail(kNullArgument, "null argument");
    if (step_from < 1 || step_from > 64 || step_to < 1 || step_to > 64)
        return fail(kInvalidQuantStep, "quantiser steps " + std::to_string(step_from) + " -> " + std::to_string(step_to) + " (both are 1..64)");
    const uint64_t sb = wide ? 2 : 1;
    if (n > UINT64_MAX / 2) return fail(kDimensionOverflow, "more symbols than memory holds");
    if (wide && (((uintptr_t)d_src | (uintptr_t)d_dst) & 1u)) return fail(kInvalidDimensions, "u16 symbols lie at even addresses");
    const uintptr_t a = (uintptr_t)d_src, b = (uintptr_t)d_dst;
    if (a != b && a < b + n * sb && b < a + n * sb) return fail(kInvalidDimensions, "source and destination overlap (in place: the same address)");
    if (!n) return kOk;
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    launch_requant_symbols(d_src, d_dst, n, wide != 0, step_from, step_to, (uint32_t*)d_hist, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}

int alice_codec_test_symbol_bins(const void* d_symbols, uint64_t n, int wide, int32_t step_from, void* d_bins, void* d_oor, void* hip_stream) {
    clear_error();
    if (!d_symbols || !d_bins || !d_oor) return fail(kNullArgument, "null argument");
    if (step_from < 1 || step_from > 64) return fail(kInvalidQuantStep, "quantiser step " + std::to_string(step_from) + " (1..64)");
    if (wide && ((uintptr_t)d_symbols & 1u)) return fail(kInvalidDimensions, "u16 symbols lie at even addresses");
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    launch_symbol_bins(d_symbols, n, wide != 0, step_from, (uint32_t*)d_bins, (uint32_t*)d_oor, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// PART 12: banded container (.alc v5; kernels: band.hip)
//
// A version 5 chunk names a base version (2, 3 or 4) whose front end, symbols and inverse it keeps; only the entropy stage
// differs: each of a channel's eight subbands is coded as a channel of the base is, with its own table.  A job is one
// (chunk, channel, band), so a call of B chunks runs 24 B jobs through one table launch, one count or decode launch and one
// scan.  The repack goes between a base chunk and its banded twin through the symbols alone.
//
// This part holds the format (header, parser, directories), the band jobs and the group bodies (band_encode_chunks,
// band_decode_chunks, to_banded_group, from_banded_group).  What a call does around its groups -- upload and download, the
// header read-back, the group loop, placement at a stride, the container checks -- is the call skeleton ahead of the
// version 2 entry points, shared with versions 2 to 4.
// ------------------------------------------------------------------------------------------

namespace {

constexpr uint32_t kBandMaxGroup = 2730;   // 24 jobs per chunk under the grid's 65 535

struct BandHeader {
    uint32_t width = 0, height = 0, frames = 0, lane_symbols = 0;
    uint8_t wavelet = 0, base = 2;
    SplitFormat fmt = kFormatSplit;   // of the base
    int32_t step[3] = {1, 1, 1}, dead_zone[3] = {1, 1, 1};
    uint32_t num_symbols[3] = {0, 0, 0}, n_blocks[24] = {};
    uint64_t payload_len[24] = {};
    uint16_t freq[24][256] = {};
};

inline const uint8_t* band_field(const uint8_t* data, int c, int k) {
    return data + kBandFixedHeaderBytes + (size_t)c * kBandChannelHeaderBytes + 12 + (size_t)k * kBandBandHeaderBytes;
}

// Header checks in their fixed order; data: at least min(total_len, kBandHeaderBytes) readable bytes of a
// container of total_len bytes.
int parse_band_header(const uint8_t* data, uint64_t total_len, BandHeader& h, ChunkDims* d) {
    if (total_len < kBandFixedHeaderBytes)
        return fail(kInvalidBitstream, "data too short for the fixed fields: " + std::to_string(total_len) + " bytes (they take " +
                                           std::to_string(kBandFixedHeaderBytes) + ")");
    if (memcmp(data, "ALCC", 4) != 0) return fail(kInvalidBitstream, "bad magic (expected ALCC)");
    if (data[4] != 5) return fail(kInvalidBitstream, "unsupported version: " + std::to_string((int)data[4]) + " (expected 5)");
    if (data[5] > 2) return fail(kInvalidBitstream, "unknown wavelet type byte: " + std::to_string((int)data[5]));
    h.wavelet = data[5];
    h.width = get_u32(data + 6); h.height = get_u32(data + 10); h.frames = get_u32(data + 14);
    h.lane_symbols = get_u32(data + 18);
    if (data[22] < 2 || data[22] > 4) return fail(kInvalidBitstream, "unknown base version: " + std::to_string((int)data[22]) + " (2, 3 or 4)");
    h.base = data[22];
    h.fmt = format_of_version(h.base);
    if (data[23] != 0) return fail(kInvalidBitstream, "reserved byte is " + std::to_string((int)data[23]) + ", not 0");
    if (!split_lane_ok(h.lane_symbols, h.fmt))
        return fail(kInvalidBitstream, "lane_symbols " + std::to_string(h.lane_symbols) + " is not a power of two in [64, " +
                                           std::to_string(is_wide(h.fmt) ? kSplitWideMaxLane : kSplitMaxLane) + "]");
    if (total_len < kBandHeaderBytes)
        return fail(kInvalidBitstream, "data too short for the header: " + std::to_string(total_len) + " bytes (minimum " + std::to_string(kBandHeaderBytes) + ")");
    *d = make_dims(h.width, h.height, h.frames);
    const unsigned __int128 pix = (unsigned __int128)h.width * h.height * h.frames;
    if (pix > UINT64_MAX / 3) return fail(kInvalidBitstream, "dimensions overflow");
    const uint64_t padded = pix == 0 ? 0 : d->padded;
    const uint64_t n_band = padded / 8;
    uint64_t total = kBandHeaderBytes;
    for (int c = 0; c < 3; ++c) {
        const uint8_t* q = data + kBandFixedHeaderBytes + (size_t)c * kBandChannelHeaderBytes;
        const std::string ch = "channel " + std::to_string(c) + ": ";
        h.step[c] = (int32_t)get_u32(q); h.dead_zone[c] = (int32_t)get_u32(q + 4);
        h.num_symbols[c] = get_u32(q + 8);
        if (h.step[c] < 1 || h.dead_zone[c] < 0)
            return fail(kInvalidBitstream, ch + "quantiser step " + std::to_string(h.step[c]) + " / dead zone " + std::to_string(h.dead_zone[c]) +
                                               " (a step is at least 1, a dead zone at least 0)");
        if ((uint64_t)h.num_symbols[c] != padded)
            return fail(kInvalidBitstream, ch + "num_symbols " + std::to_string(h.num_symbols[c]) + " != padded_pixels " + std::to_string(padded));
        for (int k = 0; k < 8; ++k) {
            const int j = 8 * c + k;
            const uint8_t* b = band_field(data, c, k);
            const std::string bk = "channel " + std::to_string(c) + " band " + std::to_string(k) + ": ";
            h.n_blocks[j] = get_u32(b);
            h.payload_len[j] = get_u64(b + 4);
            if (h.n_blocks[j] != split_blocks(n_band, h.lane_symbols))
                return fail(kInvalidBitstream, bk + "n_blocks " + std::to_string(h.n_blocks[j]) + " does not match num_symbols and lane_symbols");
            uint32_t sum = 0;
            for (int i = 0; i < 256; ++i) { h.freq[j][i] = (uint16_t)(b[12 + 2 * i] | (b[13 + 2 * i] << 8)); sum += h.freq[j][i]; }
            if (sum != (padded ? kProbScale : 0u))
                return fail(kInvalidBitstream, bk + "frequencies sum to " + std::to_string(sum) + ", not " + std::to_string(padded ? kProbScale : 0u));
            if (h.payload_len[j] < 132ull * h.n_blocks[j] || h.payload_len[j] > UINT64_MAX / 32)
                return fail(kInvalidBitstream, bk + "payload_len " + std::to_string(h.payload_len[j]) + " cannot hold its directories");
            total += h.payload_len[j];
        }
    }
    if (total != total_len)
        return fail(kInvalidBitstream, "length mismatch: header and payloads are " + std::to_string(total) + " bytes, data is " + std::to_string(total_len));
    return kOk;
}

// the block tables of a whole container in host memory
int check_band_directories(const uint8_t* data, const BandHeader& h) {
    const uint8_t* p = data + kBandHeaderBytes;
    for (int j = 0; j < 24; ++j) {
        const std::string bk = "channel " + std::to_string(j / 8) + " band " + std::to_string(j % 8) + ": ";
        uint64_t sum = 4ull * h.n_blocks[j];
        for (uint32_t b = 0; b < h.n_blocks[j]; ++b) {
            const uint32_t v = get_u32(p + 4ull * b);
            if (v < 128u) return fail(kInvalidBitstream, bk + "block " + std::to_string(b) + " is shorter than its lane directory");
            sum += v;
        }
        if (sum != h.payload_len[j])
            return fail(kInvalidBitstream, bk + "block lengths sum to " + std::to_string(sum) + ", payload_len is " + std::to_string(h.payload_len[j]));
        p += h.payload_len[j];
    }
    return kOk;
}

bool band_base_ok(uint8_t base) { return base >= 2 && base <= 4; }

uint32_t band_group(const ChunkDims& d, SplitFormat fmt) { return std::min(split_group(d, fmt), kBandMaxGroup); }

// 24 B band jobs: the channel scratch of SplitWork (one job per band) and the jobs with their geometry.  (bjobs and sent are
// declared ahead of w: w's destructor drains the stream that reads them.)
struct BandWork {
    DevBuf bjobs;
    std::vector<std::vector<SplitBandJob>> sent;
    SplitWork w;
    uint32_t pw = 0, ph = 0, hw = 0, hh = 0;
};

int band_work_alloc(BandWork& bw, uint32_t B, const ChunkDims& d, uint32_t L, bool encode, SplitFormat fmt) {
    bw.pw = (uint32_t)d.pw; bw.ph = (uint32_t)d.ph; bw.hw = bw.pw / 2; bw.hh = bw.ph / 2;
    TRY(split_work_alloc(bw.w, (int)(24 * B), d.padded / 8, L, encode, fmt));
    TRY(bw.bjobs.alloc((size_t)24 * B * sizeof(SplitBandJob)));
    return kOk;
}

// Where the bands' symbols live: chunk i, channel c at sym + (3 i + c) * padded * sb, band k at its box's origin inside.
void band_set_symbols(BandWork& bw, const uint8_t* sym, uint32_t B, const ChunkDims& d, size_t sb) {
    const uint64_t ht = d.pf / 2;
    for (uint32_t i = 0; i < B; ++i)
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 8; ++k) {
                const uint64_t origin = ((uint64_t)((k >> 2) & 1) * ht * d.ph + (uint64_t)((k >> 1) & 1) * bw.hh) * d.pw + (uint64_t)(k & 1) * bw.hw;
                bw.w.h[(size_t)24 * i + 8 * c + k].sym = sym + ((3 * (size_t)i + c) * d.padded + origin) * sb;
            }
}

int band_upload_jobs(BandWork& bw, hipStream_t st) {
    TRY(split_upload_jobs(bw.w, st));
    std::vector<SplitBandJob> v(bw.w.h.size());
    for (size_t j = 0; j < v.size(); ++j) v[j] = SplitBandJob{bw.w.h[j], bw.pw, bw.ph, bw.hw, bw.hh};
    bw.sent.push_back(std::move(v));
    HIP_TRY(hipMemcpyAsync(bw.bjobs.p, bw.sent.back().data(), bw.sent.back().size() * sizeof(SplitBandJob), hipMemcpyHostToDevice, st));
    return kOk;
}

// Whole chunks from their symbols, in two halves (as split_count_chunks / split_write_chunks): band histograms, tables (one
// launch for all 24 B), count pass and scan, sizes to the host; then the write pass and the headers.
struct BandChunkEncode {
    std::vector<BandHeaderDesc> hd;   // (declared before bw: its destructor drains the stream that reads them)
    DevBuf d_hd, hist;
    BandWork bw;
    std::vector<uint64_t> totals;
    std::vector<int32_t> steps, dead_zones;   // 3 per chunk
    ChunkDims d{};
    uint32_t B = 0, L = 0;
    uint8_t wavelet = 0, base = 2;
};

int band_count_chunks(BandChunkEncode& e, const uint8_t* sym, uint32_t B, const ChunkDims& d, uint8_t wavelet, uint32_t L, SplitFormat fmt,
                      hipStream_t st, std::vector<uint64_t>& sizes) {
    const bool wide = is_wide(fmt);
    const size_t sb = wide ? 2 : 1;
    e.B = B; e.L = L; e.d = d; e.wavelet = wavelet; e.base = format_version(fmt);
    TRY(e.hist.alloc((size_t)B * 24 * 256 * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(e.hist.p, 0, (size_t)B * 24 * 256 * sizeof(uint32_t), st));
    for (uint32_t i = 0; i < B; ++i)
        launch_band_hist(sym + (size_t)i * 3 * d.padded * sb, d, wide, e.hist.as<uint32_t>() + (size_t)i * 24 * 256, st);
    e.hd.assign(B, BandHeaderDesc{});
    BandWork& bw = e.bw;
    SplitWork& w = bw.w;
    TRY(band_work_alloc(bw, B, d, L, true, fmt));
    band_set_symbols(bw, sym, B, d, sb);
    launch_split_table(e.hist.as<uint32_t>(), w.freq.as<uint16_t>(), w.cum.as<uint16_t>(), w.n_jobs, st);
    launch_rans_tables_from_arrays(w.cum.as<uint16_t>(), w.freq.as<uint16_t>(), w.tables.as<RansTable>(), w.n_jobs, st);
    TRY(band_upload_jobs(bw, st));
    if (wide) HIP_TRY(hipMemsetAsync(w.flags.p, 0, (size_t)w.n_jobs * sizeof(uint32_t), st));
    launch_band_count(bw.bjobs.as<SplitBandJob>(), w.n_jobs, w.n_blocks, wide, st);
    launch_split_scan(w.jobs.as<SplitJob>(), w.n_jobs, false, w.totals.as<unsigned long long>(), st);
    HIP_TRY(hipGetLastError());
    e.totals.resize((size_t)w.n_jobs);
    HIP_TRY(hipMemcpyAsync(e.totals.data(), w.totals.p, e.totals.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    std::vector<uint32_t> flags;
    if (wide) {
        flags.resize((size_t)w.n_jobs);
        HIP_TRY(hipMemcpyAsync(flags.data(), w.flags.p, flags.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t j = 0; j < flags.size(); ++j)
        if (flags[j] & kSplitWideResidual)
            return fail(kInternal, "stream " + std::to_string(j) + ": a symbol above 255 + 4095 has no version 3 code");
    sizes.assign(B, kBandHeaderBytes);
    for (uint32_t i = 0; i < B; ++i)
        for (int j = 0; j < 24; ++j) sizes[i] += e.totals[(size_t)24 * i + j];
    return kOk;
}

int band_write_chunks(BandChunkEncode& e, const std::vector<uint8_t*>& outs, hipStream_t st) {
    const uint32_t B = e.B;
    SplitWork& w = e.bw.w;
    TRY(e.d_hd.alloc((size_t)B * sizeof(BandHeaderDesc)));
    for (uint32_t i = 0; i < B; ++i) {
        BandHeaderDesc& h = e.hd[i];
        h.out = outs[i];
        h.width = e.d.w; h.height = e.d.h; h.frames = e.d.f; h.lane_symbols = e.L;
        h.num_symbols = (uint32_t)e.d.padded; h.n_blocks = w.n_blocks; h.wavelet = e.wavelet; h.base = e.base;
        h.freq = w.freq.as<uint16_t>() + (size_t)i * 24 * 256;
        for (int c = 0; c < 3; ++c) { h.step[c] = e.steps[3 * (size_t)i + c]; h.dead_zone[c] = e.dead_zones[3 * (size_t)i + c]; }
        uint64_t off = kBandHeaderBytes;
        for (int j = 0; j < 24; ++j) {
            h.payload_len[j] = e.totals[(size_t)24 * i + j];
            w.h[(size_t)24 * i + j].stream = outs[i] + off;
            off += h.payload_len[j];
        }
    }
    HIP_TRY(hipMemcpyAsync(e.d_hd.p, e.hd.data(), e.hd.size() * sizeof(BandHeaderDesc), hipMemcpyHostToDevice, st));
    TRY(band_upload_jobs(e.bw, st));
    launch_band_write(e.bw.bjobs.as<SplitBandJob>(), w.n_jobs, w.n_blocks, w.wide, st);
    launch_band_headers(e.d_hd.as<BandHeaderDesc>(), (int)B, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}

// B equal-shaped chunks from pixels: the base's forward pass (its fused channel histogram is not used), then the halves above.
template <typename Place>
int band_encode_chunks(const RgbLayout* rgb, uint32_t B, const ChunkDims& d, uint8_t wavelet, const uint8_t* q, uint32_t L, SplitFormat fmt,
                       hipStream_t st, std::vector<uint64_t>& sizes, Place place) {
    const bool wide = is_wide(fmt);
    const size_t sb = wide ? 2 : 1;
    EncodeWork ew;
    BandChunkEncode e;     // (after ew: its destructor drains the stream that reads ew.sym)
    ew.d = d; ew.n_chunks = (int)B;
    if (transform_tiles_eligible(d)) TRY(ew.scratch.alloc(forward_scratch_bytes(d)));
    TRY(ew.sym.alloc((size_t)B * 3 * d.padded * sb));
    TRY(ew.hist.alloc((size_t)B * 3 * 256 * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(ew.hist.p, 0, (size_t)B * 3 * 256 * sizeof(uint32_t), st));
    StreamDrain drain(st);
    e.steps.resize(3 * (size_t)B); e.dead_zones.resize(3 * (size_t)B);
    for (uint32_t i = 0; i < B; ++i) {
        const int32_t step = quality_to_step(q[i]);
        for (int c = 0; c < 3; ++c) e.steps[3 * (size_t)i + c] = e.dead_zones[3 * (size_t)i + c] = step;
        TRY(forward_chunk(rgb[i], d, wavelet, step, ew, ew.sym.as<uint8_t>() + (size_t)i * 3 * d.padded * sb,
                          ew.hist.as<uint32_t>() + (size_t)i * 3 * 256, st, wide));
    }
    TRY(band_count_chunks(e, ew.sym.as<uint8_t>(), B, d, wavelet, L, fmt, st, sizes));
    std::vector<uint8_t*> outs(B, nullptr);
    TRY(place(sizes, outs));
    return band_write_chunks(e, outs, st);
}

// Queues the tables, the directory scan and the band decode of B chunks (hdr[i] validated, d_alc[i] the chunk's first byte on
// the device) into the symbol volumes at sym (chunk stride 3 * padded * sb); split_decode_verdict(bw.w, st) reads the flags.
int band_decode_launch(BandWork& bw, const BandHeader* hdr, const uint8_t* const* d_alc, uint32_t B, const ChunkDims& d, uint8_t* sym,
                       hipStream_t st) {
    const SplitFormat fmt = hdr[0].fmt;
    const size_t sb = is_wide(fmt) ? 2 : 1;
    TRY(band_work_alloc(bw, B, d, hdr[0].lane_symbols, false, fmt));
    SplitWork& w = bw.w;
    w.st = st; w.armed = true;
    band_set_symbols(bw, sym, B, d, sb);
    w.h_freq.resize((size_t)w.n_jobs * 256);
    w.h_cum.assign((size_t)w.n_jobs * 256, 0);
    for (uint32_t i = 0; i < B; ++i) {
        uint64_t off = kBandHeaderBytes;
        for (int j = 0; j < 24; ++j) {
            const size_t t = (size_t)24 * i + j;
            memcpy(&w.h_freq[t * 256], hdr[i].freq[j], 256 * sizeof(uint16_t));
            uint32_t run = 0;
            for (int s = 0; s < 256; ++s) { w.h_cum[t * 256 + s] = (uint16_t)run; run += hdr[i].freq[j][s]; }
            w.h[t].stream = (uint8_t*)d_alc[i] + off;
            w.h[t].len = hdr[i].payload_len[j];
            off += hdr[i].payload_len[j];
        }
    }
    HIP_TRY(hipMemcpyAsync(w.freq.p, w.h_freq.data(), w.h_freq.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(w.cum.p, w.h_cum.data(), w.h_cum.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(w.flags.p, 0, (size_t)w.n_jobs * sizeof(uint32_t), st));
    TRY(band_upload_jobs(bw, st));
    launch_rans_tables_from_arrays(w.cum.as<uint16_t>(), w.freq.as<uint16_t>(), w.tables.as<RansTable>(), w.n_jobs, st);
    launch_split_scan(w.jobs.as<SplitJob>(), w.n_jobs, true, nullptr, st);
    launch_band_decode(bw.bjobs.as<SplitBandJob>(), w.n_jobs, w.n_blocks, w.wide, st);
    HIP_TRY(hipGetLastError());
    return kOk;
}

// Decode of B equal-shaped chunks of one base to pixels at rgb[i]: straight into the volume the base's inverse reads.
// Returns after the stream has drained, with the verdict of the end checks.
int band_decode_chunks(const BandHeader* hdr, const uint8_t* const* d_alc, uint32_t B, const ChunkDims& d, const RgbLayout* rgb, hipStream_t st) {
    DecodeWork dw;
    dw.d = d; dw.n_chunks = (int)B;
    const SplitFormat fmt = hdr[0].fmt;
    const bool wide = is_wide(fmt);
    const size_t sb = wide ? 2 : 1;
    TRY(dw.sym.alloc((size_t)B * 3 * d.padded * sb));
    bool any16 = false, any32 = false;
    for (uint32_t i = 0; i < B; ++i) (inverse_bounds(hdr[i].wavelet, hdr[i].step, wide ? kWideMaxQ : kByteMaxQ).mid16 ? any16 : any32) = true;
    if (transform_tiles_eligible(d)) TRY(dw.scratch_own.alloc(group_scratch_bytes(d, any16, any32)));
    BandWork bw;   // (after dw: its destructor drains the stream)
    TRY(band_decode_launch(bw, hdr, d_alc, B, d, dw.sym.as<uint8_t>(), st));
    for (uint32_t i = 0; i < B; ++i)
        TRY(inverse_chunk(dw.sym.as<uint8_t>() + (size_t)i * 3 * d.padded * sb, d, hdr[i].wavelet, hdr[i].step, dw.scratch_own.p, dw, rgb[i], st, fmt));
    HIP_TRY(hipGetLastError());
    return split_decode_verdict(bw.w, st);
}

// The headers of n device containers, read back and validated; the chunks agree in base, wavelet, shape and lane_symbols.
int band_device_headers(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks, hipStream_t st,
                        std::vector<BandHeader>& hdr, std::vector<const uint8_t*>& ptr, ChunkDims& d) {
    return read_device_headers(d_alc, alc_stride, sizes, n_chunks, kBandHeaderBytes, st,
                               [](const uint8_t* raw, uint64_t size, BandHeader& h, ChunkDims& di) { return parse_band_header(raw, size, h, &di); },
                               [](const BandHeader& h0, const BandHeader& hi) {
                                   return hi.base == h0.base && hi.wavelet == h0.wavelet && hi.lane_symbols == h0.lane_symbols;
                               },
                               "the chunks of one call must have the same base, wavelet, shape and lane_symbols", hdr, ptr, d);
}

// ---- repack: between a base chunk and its banded twin through the symbols, no transform ----

// One group base -> banded: lane decode of every block into the symbol volume (its verdict first: nothing of a damaged
// source is coded), then the encode from symbols.
template <typename Place>
int to_banded_group(const SplitHeader* hdr, const uint8_t* const* d_alc, uint32_t B, const ChunkDims& d, uint32_t L, hipStream_t st,
                    std::vector<uint64_t>& sizes, Place place) {
    TranscodeSource s;
    BandChunkEncode e;     // (after s: its destructor drains the stream that reads s.sym)
    TRY(transcode_decode(s, hdr, d_alc, B, d, st));
    e.steps.resize(3 * (size_t)B); e.dead_zones.resize(3 * (size_t)B);
    for (uint32_t i = 0; i < B; ++i)
        for (int c = 0; c < 3; ++c) { e.steps[3 * (size_t)i + c] = hdr[i].step[c]; e.dead_zones[3 * (size_t)i + c] = hdr[i].dead_zone[c]; }
    TRY(band_count_chunks(e, s.sym.as<uint8_t>(), B, d, hdr[0].wavelet, L, hdr[0].fmt, st, sizes));
    std::vector<uint8_t*> outs(B, nullptr);
    TRY(place(sizes, outs));
    return band_write_chunks(e, outs, st);
}

// One group banded -> base: band decode into the symbol volume, a 256-bin count of each channel, then the base's own table,
// count and write passes (the first half of an encode from symbols at a target step that leaves every channel untouched).
template <typename Place>
int from_banded_group(const BandHeader* hdr, const uint8_t* const* d_alc, uint32_t B, const ChunkDims& d, uint32_t L, hipStream_t st,
                      std::vector<uint64_t>& sizes, Place place) {
    const SplitFormat fmt = hdr[0].fmt;
    const size_t sb = is_wide(fmt) ? 2 : 1;
    DevBuf sym;
    StreamDrain drain(st);
    SplitChunkEncode e;
    TRY(sym.alloc((size_t)B * 3 * d.padded * sb));
    {
        BandWork bw;
        TRY(band_decode_launch(bw, hdr, d_alc, B, d, sym.as<uint8_t>(), st));
        TRY(split_decode_verdict(bw.w, st));
    }
    std::vector<SplitHeader> sh(B);
    std::vector<int32_t> keep(B, 1);
    for (uint32_t i = 0; i < B; ++i) {
        sh[i].fmt = fmt; sh[i].wavelet = hdr[i].wavelet;
        for (int c = 0; c < 3; ++c) { sh[i].step[c] = hdr[i].step[c]; sh[i].dead_zone[c] = hdr[i].dead_zone[c]; }
    }
    TRY(transcode_count_chunks(e, sym.as<uint8_t>(), sym.as<uint8_t>(), sh.data(), B, d, keep.data(), L, fmt, st, sizes));
    std::vector<uint8_t*> outs(B, nullptr);
    TRY(place(sizes, outs));
    return split_write_chunks(e, outs, st);
}

void write_empty_banded(uint8_t* p, uint8_t wavelet, uint32_t w, uint32_t h, uint32_t f, uint32_t L, uint8_t base, const int32_t* step,
                        const int32_t* dead_zone) {
    memset(p, 0, kBandHeaderBytes);
    memcpy(p, "ALCC", 4);
    p[4] = 5; p[5] = wavelet;
    put_u32(p + 6, w); put_u32(p + 10, h); put_u32(p + 14, f); put_u32(p + 18, L);
    p[22] = base;
    for (int c = 0; c < 3; ++c) {
        uint8_t* q = p + kBandFixedHeaderBytes + (size_t)c * kBandChannelHeaderBytes;
        put_u32(q, (uint32_t)step[c]); put_u32(q + 4, (uint32_t)dead_zone[c]);
    }
}

int band_check_base_lane(uint8_t base, uint32_t lane_symbols, uint32_t* L, SplitFormat* fmt) {
    if (!band_base_ok(base)) return fail(kInvalidDimensions, "base " + std::to_string((int)base) + " (a banded chunk has base 2, 3 or 4)");
    *fmt = format_of_version(base);
    *L = lane_symbols ? lane_symbols : kSplitDefaultLane;
    if (!split_lane_ok(*L, *fmt)) return fail(kInvalidDimensions, split_lane_msg(*fmt));
    return kOk;
}

}  // namespace

extern "C" {

uint64_t alice_codec_banded_stream_bound(uint64_t n_band, uint32_t lane_symbols, uint8_t base) {
    if (!band_base_ok(base) || !split_lane_ok(lane_symbols, format_of_version(base)) || n_band > 0xFFFFFFFFull / 8) return 0;
    return (uint64_t)split_blocks(n_band, lane_symbols) * (4 + 128 + 64 * 4) + (base == 2 ? 2 : 4) * n_band;
}

int alice_codec_banded_info(const uint8_t* data, uint64_t len, AliceBandedInfo* info) {
    clear_error();
    if (!data || !info) return fail(kNullArgument, "null argument");
    BandHeader h;
    ChunkDims d{};
    TRY(parse_band_header(data, len, h, &d));
    TRY(check_band_directories(data, h));
    memset(info, 0, sizeof(*info));
    info->width = h.width; info->height = h.height; info->frames = h.frames;
    info->lane_symbols = h.lane_symbols; info->wavelet = h.wavelet; info->base = h.base;
    for (int c = 0; c < 3; ++c) { info->quant_step[c] = h.step[c]; info->dead_zone[c] = h.dead_zone[c]; info->num_symbols[c] = h.num_symbols[c]; }
    for (int j = 0; j < 24; ++j) { info->n_blocks[j] = h.n_blocks[j]; info->payload_len[j] = h.payload_len[j]; }
    return kOk;
}

uint8_t* alice_codec_encode_banded(const FrameEncoder* encoder, const uint8_t* rgb, uint64_t rgb_len, uint32_t width, uint32_t height,
                                   uint32_t frames, uint32_t lane_symbols, uint8_t base, uint64_t* out_len) {
    clear_error();
    if (!encoder || !rgb || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    auto run = [&](uint8_t** out) -> int {
        uint64_t n_pixels = 0;
        TRY(checked_pixel_count(width, height, frames, &n_pixels));
        if (n_pixels == 0 && rgb_len != 0) return fail(kInvalidBufferSize, "buffer size mismatch: expected 0, got " + std::to_string(rgb_len));
        ChunkDims d{};
        EncodedChunk* none = nullptr;
        if (n_pixels) TRY(validate_encode_many(encoder, rgb, rgb_len, width, height, frames, 1, &none, &d));
        uint32_t L = 0;
        SplitFormat fmt;
        TRY(band_check_base_lane(base, lane_symbols, &L, &fmt));
        if (n_pixels == 0)
            return host_header_result(kBandHeaderBytes, out, out_len, [&](uint8_t* p) {
                const int32_t s = quality_to_step(encoder->quality), steps[3] = {s, s, s};
                write_empty_banded(p, encoder->wavelet, width, height, frames, L, base, steps, steps);
            });
        return host_one_result(rgb, n_pixels * 3, out, out_len, [&](const uint8_t* d_rgb, hipStream_t st, std::vector<uint64_t>& sizes, auto place) {
            const RgbLayout layout = packed_rgb(d_rgb, d);
            return band_encode_chunks(&layout, 1, d, encoder->wavelet, &encoder->quality, L, fmt, st, sizes, place);
        });
    };
    uint8_t* out = nullptr;
    return run(&out) == kOk ? out : nullptr;
}

uint8_t* alice_codec_decode_banded(const uint8_t* data, uint64_t len, uint64_t* out_len) {
    clear_error();
    if (!data || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    auto run = [&](uint8_t** out) -> int {
        BandHeader h;
        ChunkDims d{};
        TRY(parse_band_header(data, len, h, &d));
        TRY(check_band_directories(data, h));
        return host_decode_pixels(data, len, (uint64_t)h.width * h.height * h.frames * 3, out, out_len,
                                  [&](const uint8_t* d_alc, void* d_rgb, hipStream_t st) {
                                      const RgbLayout layout = packed_rgb(d_rgb, d);
                                      return band_decode_chunks(&h, &d_alc, 1, d, &layout, st);
                                  });
    };
    uint8_t* out = nullptr;
    return run(&out) == kOk ? out : nullptr;
}

int alice_codec_dev_encode_banded(const void* d_rgb, uint32_t width, uint32_t height, uint32_t frames, uint32_t n_chunks,
                                  uint8_t wavelet_type, uint8_t quality, const uint8_t* qualities, uint32_t lane_symbols, uint8_t base,
                                  void* d_out, uint64_t out_stride, uint64_t* sizes, void* hip_stream) {
    clear_error();
    if (!d_rgb || !d_out || !sizes) return fail(kNullArgument, "null argument");
    if (wavelet_type > 2) return fail(kInvalidBitstream, "unknown wavelet type");
    ChunkDims d{};
    TRY(chunk_dims(width, height, frames, &d, n_chunks));
    uint32_t L = 0;
    SplitFormat fmt;
    TRY(band_check_base_lane(base, lane_symbols, &L, &fmt));
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    std::vector<RgbLayout> layouts(n_chunks);
    std::vector<uint8_t> q(n_chunks);
    for (uint32_t i = 0; i < n_chunks; ++i) {
        layouts[i] = packed_rgb((const uint8_t*)d_rgb + (size_t)i * d.n_pixels * 3, d);
        q[i] = qualities ? qualities[i] : quality;
    }
    return for_each_group(n_chunks, band_group(d, fmt), sizes, [&](uint32_t first, uint32_t B, std::vector<uint64_t>& sz) {
        return band_encode_chunks(layouts.data() + first, B, d, wavelet_type, q.data() + first, L, fmt, st, sz, place_strided(d_out, out_stride, first, B));
    });
}

int alice_codec_dev_decode_banded(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks, void* d_rgb_out,
                                  void* hip_stream) {
    clear_error();
    if (!d_rgb_out) return fail(kNullArgument, "null argument");
    TRY(check_dev_containers(d_alc, alc_stride, sizes, n_chunks));
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    std::vector<BandHeader> hdr;
    std::vector<const uint8_t*> ptr;
    ChunkDims d{};
    TRY(band_device_headers(d_alc, alc_stride, sizes, n_chunks, st, hdr, ptr, d));
    std::vector<RgbLayout> layouts;
    TRY(split_layouts(d_rgb_out, 0, 0, nullptr, d, n_chunks, layouts));
    return for_each_group(n_chunks, band_group(d, hdr[0].fmt), nullptr, [&](uint32_t first, uint32_t B, std::vector<uint64_t>&) {
        return band_decode_chunks(hdr.data() + first, ptr.data() + first, B, d, layouts.data() + first, st);
    });
}

uint8_t* alice_codec_to_banded(const uint8_t* data, uint64_t len, uint32_t lane_symbols, uint64_t* out_len) {
    clear_error();
    if (!data || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    auto run = [&](uint8_t** out) -> int {
        SplitHeader h;
        ChunkDims d{};
        TRY(frames_validate_header(data, len, h, d));
        const uint32_t L = lane_symbols ? lane_symbols : h.lane_symbols;
        if (!split_lane_ok(L, h.fmt)) return fail(kInvalidDimensions, split_lane_msg(h.fmt));
        TRY(check_split_directories(data, h));
        if (d.n_pixels == 0)
            return host_header_result(kBandHeaderBytes, out, out_len, [&](uint8_t* p) {
                write_empty_banded(p, h.wavelet, h.width, h.height, h.frames, L, format_version(h.fmt), h.step, h.dead_zone);
            });
        return host_one_result(data, len, out, out_len, [&](const uint8_t* d_alc, hipStream_t st, std::vector<uint64_t>& sizes, auto place) {
            return to_banded_group(&h, &d_alc, 1, d, L, st, sizes, place);
        });
    };
    uint8_t* out = nullptr;
    return run(&out) == kOk ? out : nullptr;
}

uint8_t* alice_codec_from_banded(const uint8_t* data, uint64_t len, uint32_t lane_symbols, uint64_t* out_len) {
    clear_error();
    if (!data || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    auto run = [&](uint8_t** out) -> int {
        BandHeader h;
        ChunkDims d{};
        TRY(parse_band_header(data, len, h, &d));
        const uint32_t L = lane_symbols ? lane_symbols : h.lane_symbols;
        if (!split_lane_ok(L, h.fmt)) return fail(kInvalidDimensions, split_lane_msg(h.fmt));
        TRY(check_band_directories(data, h));
        if (d.n_pixels == 0)
            return host_header_result(kSplitHeaderBytes, out, out_len, [&](uint8_t* p) {
                write_empty_split(p, h.wavelet, h.width, h.height, h.frames, L, h.step[0], h.base);
                for (int c = 0; c < 3; ++c) {
                    uint8_t* q = p + kSplitFixedHeaderBytes + (size_t)c * kSplitChannelHeaderBytes;
                    put_u32(q, (uint32_t)h.step[c]); put_u32(q + 4, (uint32_t)h.dead_zone[c]);
                }
            });
        return host_one_result(data, len, out, out_len, [&](const uint8_t* d_alc, hipStream_t st, std::vector<uint64_t>& sizes, auto place) {
            return from_banded_group(&h, &d_alc, 1, d, L, st, sizes, place);
        });
    };
    uint8_t* out = nullptr;
    return run(&out) == kOk ? out : nullptr;
}

int alice_codec_dev_to_banded(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks, uint32_t lane_symbols,
                              void* d_out, uint64_t out_stride, uint64_t* out_sizes, void* hip_stream) {
    clear_error();
    if (!d_out || !out_sizes) return fail(kNullArgument, "null argument");
    TRY(check_dev_containers(d_alc, alc_stride, sizes, n_chunks));
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    std::vector<SplitHeader> hdr;
    std::vector<const uint8_t*> ptr;
    ChunkDims d{};
    TRY(source_device_headers(d_alc, alc_stride, sizes, n_chunks, st, hdr, ptr, d));
    const uint32_t L = lane_symbols ? lane_symbols : hdr[0].lane_symbols;
    if (!split_lane_ok(L, hdr[0].fmt)) return fail(kInvalidDimensions, split_lane_msg(hdr[0].fmt));
    return for_each_group(n_chunks, band_group(d, hdr[0].fmt), out_sizes, [&](uint32_t first, uint32_t B, std::vector<uint64_t>& sz) {
        return to_banded_group(hdr.data() + first, ptr.data() + first, B, d, L, st, sz, place_strided(d_out, out_stride, first, B));
    });
}

int alice_codec_dev_from_banded(const void* d_alc, uint64_t alc_stride, const uint64_t* sizes, uint32_t n_chunks, uint32_t lane_symbols,
                                void* d_out, uint64_t out_stride, uint64_t* out_sizes, void* hip_stream) {
    clear_error();
    if (!d_out || !out_sizes) return fail(kNullArgument, "null argument");
    TRY(check_dev_containers(d_alc, alc_stride, sizes, n_chunks));
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    std::vector<BandHeader> hdr;
    std::vector<const uint8_t*> ptr;
    ChunkDims d{};
    TRY(band_device_headers(d_alc, alc_stride, sizes, n_chunks, st, hdr, ptr, d));
    const uint32_t L = lane_symbols ? lane_symbols : hdr[0].lane_symbols;
    if (!split_lane_ok(L, hdr[0].fmt)) return fail(kInvalidDimensions, split_lane_msg(hdr[0].fmt));
    return for_each_group(n_chunks, band_group(d, hdr[0].fmt), out_sizes, [&](uint32_t first, uint32_t B, std::vector<uint64_t>& sz) {
        return from_banded_group(hdr.data() + first, ptr.data() + first, B, d, L, st, sz, place_strided(d_out, out_stride, first, B));
    });
}

int alice_codec_dev_band_histograms(const void* d_symbols, uint32_t width, uint32_t height, uint32_t frames, int wide, void* d_hist,
                                    void* hip_stream) {
    clear_error();
    if (!d_symbols || !d_hist) return fail(kNullArgument, "null argument");
    ChunkDims d{};
    TRY(chunk_dims(width, height, frames, &d));
    if (wide && ((uintptr_t)d_symbols & 1u)) return fail(kInvalidDimensions, "u16 symbols lie at even addresses");
    if ((uintptr_t)d_hist & 3u) return fail(kInvalidDimensions, "the histograms lie at a multiple of 4 bytes");
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    HIP_TRY(hipMemsetAsync(d_hist, 0, 3 * 8 * 256 * sizeof(uint32_t), st));
    launch_band_hist(d_symbols, d, wide != 0, (uint32_t*)d_hist, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return kOk;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// PART 13: frame ranges and half-size previews of a banded chunk (kernels: band_range_decode_kernel of
// band.hip, the finishes of PART 8 and PART 9 unchanged)
//
// A band's symbols are the raster [t''][y''][x''] of its octant, so the coefficient planes t'' in [a/2, b/2) of a band are ONE
// run of band-order symbols, [a/2 Q, b/2 Q) with Q = hw hh, and that run and the blocks that hold it are the same for every
// band and channel.  A frame range keeps the run of all eight bands and stores it where the virtual chunk of b - a frames has
// that band (the volume inverse_window reads); a preview keeps bands 0 and 4 alone, which ARE the low-low quadrants of the
// window's planes, and stores them as the compact volume launch_preview_inverse reads.  The windows, the output sizes, the
// range checks and both finishes are PART 8's and PART 9's.
// ------------------------------------------------------------------------------------------

namespace {

enum BandPartialKind : int { kBandFrames = 0, kBandPreview = 1 };

struct BandPartialPlan {
    uint32_t a = 0, b = 0;                   // section 14.1's window
    uint32_t idx_lo = 0, idx_hi = 0;         // the kept band-order indices of every kept band
    uint32_t blk_first = 0, blk_count = 0;   // the planned blocks of every kept band
    bool kept[8] = {};
    uint32_t n_kept = 0;                     // bands per channel
    uint64_t stored = 0;                     // symbols of a channel that are stored
};

BandPartialPlan band_partial_plan(BandPartialKind kind, const BandHeader& h, const ChunkDims& d, uint32_t first, uint32_t count) {
    BandPartialPlan p;
    axis_window(frames_halo(h.wavelet), d.pf, first, (uint64_t)first + count, &p.a, &p.b);
    const uint64_t Q = (d.pw / 2) * (d.ph / 2), B = 64ull * h.lane_symbols;
    p.idx_lo = (uint32_t)(p.a / 2 * Q); p.idx_hi = (uint32_t)(p.b / 2 * Q);    // at most n_band < 2^29
    p.blk_first = (uint32_t)(p.idx_lo / B);
    p.blk_count = (uint32_t)((p.idx_hi + B - 1) / B) - p.blk_first;
    for (int k = 0; k < 8; ++k) p.kept[k] = kind == kBandFrames || (k & 3) == 0;
    p.n_kept = kind == kBandFrames ? 8u : 2u;
    p.stored = (uint64_t)(p.b - p.a) * (kind == kBandFrames ? d.pw * d.ph : Q);
    return p;
}

// What the calling thread's last call of each kind planned and did: the test hooks of alice_codec_test.h read these
struct BandPartialStats { uint64_t a, b, blocks, uploaded, frames, stored; };
thread_local BandPartialStats tl_band_partial_stats[2] = {};

int band_partial_done(BandPartialKind kind, const BandPartialPlan& p, uint32_t count, uint64_t uploaded, hipStream_t st) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    tl_band_partial_stats[kind] = BandPartialStats{p.a, p.b, 3ull * p.n_kept * p.blk_count, uploaded, count, 3 * p.stored};
    return kOk;
}

// The checks of the four calls after the null checks: the header in section 20.3's order, then the range as PART 8 has it
int band_partial_validate(const uint8_t* data, uint64_t len, uint32_t first, uint32_t count, BandHeader& h, ChunkDims& d) {
    TRY(parse_band_header(data, len, h, &d));
    SplitHeader range;
    range.frames = h.frames;
    return frames_validate_range(range, d, first, count);
}

// The lane stage: the planned blocks of the kept bands of the container at d_alc (device, h validated) are decoded and the
// kept run of channel c, band k stored at d_sym + (c * chan_stride + origin[k]) symbols with the pitches given.  All jobs
// (the 24 scan jobs and the range jobs behind them) go up in one copy while nothing of the call is queued yet; the scan runs
// over all 24 block-length tables, so a corrupt entry is refused wherever it is; the verdict of the end checks comes before
// the caller queues anything that writes its output.  Stream numbers in a verdict are 8 channel + band.
struct BandLaneStage {
    DevBuf jobs;                 // (before w: w's destructor drains the stream that reads them)
    std::vector<uint8_t> up;
    SplitWork w;
};

int band_partial_lane_decode(BandLaneStage& ls, const BandHeader& h, const ChunkDims& d, const BandPartialPlan& p, const uint8_t* d_alc,
                             uint8_t* d_sym, uint64_t chan_stride, const uint64_t origin[8], uint64_t row_pitch, uint64_t plane_pitch,
                             hipStream_t st) {
    const bool wide = is_wide(h.fmt);
    const size_t sb = wide ? 2 : 1;
    const uint32_t n_range = 3 * p.n_kept;
    SplitWork& w = ls.w;
    TRY(split_work_alloc(w, 24, d.padded / 8, h.lane_symbols, false, h.fmt));
    const size_t range_at = 24 * sizeof(SplitJob);
    static_assert(sizeof(SplitJob) % alignof(SplitBandRangeJob) == 0, "the range jobs lie behind the scan jobs");
    ls.up.resize(range_at + n_range * sizeof(SplitBandRangeJob));
    TRY(ls.jobs.alloc(ls.up.size()));
    // the kept bands' tables are w.tables[0 .. n_range), in job order
    w.h_freq.assign((size_t)n_range * 256, 0);
    w.h_cum.assign((size_t)n_range * 256, 0);
    uint64_t off = kBandHeaderBytes;
    uint32_t r = 0;
    for (int j = 0; j < 24; ++j) {
        SplitJob& s = w.h[(size_t)j];
        const int c = j / 8, k = j % 8;
        s.stream = (uint8_t*)d_alc + off;
        s.len = h.payload_len[j];
        off += h.payload_len[j];
        s.sym = nullptr;
        if (!p.kept[k]) continue;
        memcpy(&w.h_freq[(size_t)r * 256], h.freq[j], 256 * sizeof(uint16_t));
        uint32_t run = 0;
        for (int i = 0; i < 256; ++i) { w.h_cum[(size_t)r * 256 + i] = (uint16_t)run; run += h.freq[j][i]; }
        SplitBandRangeJob rj{};
        rj.j = s;
        rj.j.table = w.tables.as<RansTable>() + r;
        rj.j.sym = d_sym + ((size_t)c * chan_stride + origin[k]) * sb;
        rj.hw = (uint32_t)(d.pw / 2); rj.hh = (uint32_t)(d.ph / 2);
        rj.row_pitch = row_pitch; rj.plane_pitch = plane_pitch;
        rj.blk_first = p.blk_first; rj.blk_count = p.blk_count;
        rj.idx_lo = p.idx_lo; rj.idx_hi = p.idx_hi;
        memcpy(ls.up.data() + range_at + (size_t)r * sizeof(rj), &rj, sizeof(rj));
        ++r;
    }
    memcpy(ls.up.data(), w.h.data(), range_at);
    w.st = st; w.armed = true;
    HIP_TRY(hipMemcpyAsync(ls.jobs.p, ls.up.data(), ls.up.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(w.freq.p, w.h_freq.data(), w.h_freq.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(w.cum.p, w.h_cum.data(), w.h_cum.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(w.flags.p, 0, 24 * sizeof(uint32_t), st));
    launch_rans_tables_from_arrays(w.cum.as<uint16_t>(), w.freq.as<uint16_t>(), w.tables.as<RansTable>(), (int)n_range, st);
    launch_split_scan(ls.jobs.as<SplitJob>(), 24, true, nullptr, st);
    launch_band_range_decode((const SplitBandRangeJob*)(ls.jobs.as<uint8_t>() + range_at), (int)n_range, p.blk_count, wide, st);
    HIP_TRY(hipGetLastError());
    return split_decode_verdict(w, st);
}

// Frames [first, first + count) of the banded container at d_alc (device; h and the range validated) to `out`.  The kept runs
// are the symbol volume of the virtual chunk of b - a frames (rect_decode_device's whole-frame case); returns after the
// stream has drained.
int band_frames_decode_device(const BandHeader& h, const ChunkDims& d, const BandPartialPlan& p, const uint8_t* d_alc, uint32_t first,
                              uint32_t count, const RgbLayout& out, hipStream_t st, uint64_t uploaded) {
    const bool wide = is_wide(h.fmt);
    const size_t sb = wide ? 2 : 1;
    const ChunkDims dv = make_dims(h.width, h.height, p.b - p.a);
    const ChunkDims dx = make_dims(dv.w, dv.h, count);
    DecodeWork dw;
    dw.d = dv; dw.n_chunks = 1;
    TRY(dw.sym.alloc(3 * dv.padded * sb));
    if (transform_tiles_eligible(dv))
        TRY(dw.scratch_own.alloc(inverse_scratch_bytes(dx, inverse_bounds(h.wavelet, h.step, wide ? kWideMaxQ : kByteMaxQ).mid16)));
    const uint64_t hw = d.pw / 2, hh = d.ph / 2, half = (p.b - p.a) / 2;
    uint64_t origin[8];
    for (int k = 0; k < 8; ++k) origin[k] = ((uint64_t)((k >> 2) & 1) * half * d.ph + (uint64_t)((k >> 1) & 1) * hh) * d.pw + (uint64_t)(k & 1) * hw;
    BandLaneStage ls;
    TRY(band_partial_lane_decode(ls, h, d, p, d_alc, dw.sym.as<uint8_t>(), dv.padded, origin, d.pw, d.pw * d.ph, st));
    TRY(inverse_window(dw.sym.as<uint8_t>(), dv, first - p.a, first - p.a + count, h.wavelet, h.step, dw.scratch_own.p, dw, out, st, h.fmt));
    return band_partial_done(kBandFrames, p, count, uploaded, st);
}

// The preview of frames [first, first + count) of the banded container at d_alc to d_rgb (count * hh * hw * 3 bytes): bands 0
// and 4 as the compact volume [ch][b - a][pitch] of PART 9.  Returns after the stream has drained.
int band_preview_decode_device(const BandHeader& h, const ChunkDims& d, const BandPartialPlan& p, const uint8_t* d_alc, uint32_t first,
                               uint32_t count, void* d_rgb, hipStream_t st, uint64_t uploaded) {
    const bool wide = is_wide(h.fmt);
    const size_t sb = wide ? 2 : 1;
    const uint32_t planes = p.b - p.a;
    const uint64_t hw = d.pw / 2, quadrant = hw * (d.ph / 2), pitch = round_up(quadrant, 4);
    // (the pad symbols of a plane are never stored and need no value: preview_decode_device)
    DevBuf d_sym;
    TRY(d_sym.alloc(3 * (size_t)planes * pitch * sb));
    uint64_t origin[8] = {};
    origin[4] = (uint64_t)(planes / 2) * pitch;
    BandLaneStage ls;
    TRY(band_partial_lane_decode(ls, h, d, p, d_alc, d_sym.as<uint8_t>(), (uint64_t)planes * pitch, origin, hw, pitch, st));
    const InverseBounds ib = inverse_bounds(h.wavelet, h.step, wide ? kWideMaxQ : kByteMaxQ);
    if (!launch_preview_inverse(d_sym.p, pitch, quadrant, planes, FrameWindow{first - p.a, first - p.a + count}, (int)h.fmt, h.wavelet, h.step,
                                ib.exact, (uint8_t*)d_rgb, st))
        return fail(kInternal, "preview: no finish kernel for this volume");
    return band_partial_done(kBandPreview, p, count, uploaded, st);
}

// The spans of a banded container in host memory that go up for a plan: the header, the 24 block-length tables (with
// section 20.3's directory checks applied to all of them on the way) and, per kept band, the one byte run of its planned blocks.
int band_partial_spans(const uint8_t* data, const BandHeader& h, const BandPartialPlan& p, std::vector<PartialSpan>& spans,
                       uint64_t& payload_bytes) {
    spans.push_back({0, kBandHeaderBytes});
    uint64_t pos = kBandHeaderBytes;
    payload_bytes = 0;
    for (int j = 0; j < 24; ++j) {
        const std::string bk = "channel " + std::to_string(j / 8) + " band " + std::to_string(j % 8) + ": ";
        const uint8_t* tab = data + pos;
        const uint32_t nb = h.n_blocks[j];
        uint64_t sum = 4ull * nb, run_off = 0, run_len = 0;
        for (uint32_t blk = 0; blk < nb; ++blk) {
            const uint32_t v = get_u32(tab + 4ull * blk);
            if (v < 128u) return fail(kInvalidBitstream, bk + "block " + std::to_string(blk) + " is shorter than its lane directory");
            if (blk == p.blk_first) run_off = sum;
            if (blk - p.blk_first < p.blk_count) run_len += v;
            sum += v;
        }
        if (sum != h.payload_len[j])
            return fail(kInvalidBitstream, bk + "block lengths sum to " + std::to_string(sum) + ", payload_len is " + std::to_string(h.payload_len[j]));
        spans.push_back({pos, 4ull * nb});
        if (p.kept[j % 8] && run_len) {      // (inside the payload: the lengths sum to it)
            spans.push_back({pos + run_off, run_len});
            payload_bytes += run_len;
        }
        pos += h.payload_len[j];
    }
    return kOk;
}

// The host calls: validated header and plan, the spans to their own offsets of a pool buffer of the container's size, the
// device path on it, the result down.  device(d_alc, d_rgb, stream, uploaded payload bytes) decodes `bytes` bytes to d_rgb.
template <typename Device>
int band_partial_decode_host(const uint8_t* data, uint64_t len, const BandHeader& h, const BandPartialPlan& p, uint64_t bytes, uint8_t** result,
                             uint64_t* out_len, Device device) {
    std::vector<PartialSpan> spans;
    uint64_t payload_bytes = 0;
    TRY(band_partial_spans(data, h, p, spans, payload_bytes));
    std::unique_ptr<uint8_t, decltype(&free)> out(host_result_alloc(bytes), &free);   // freed on every failure below
    if (!out) return fail(kOutOfMemory, "out of host memory");
    hipStream_t st;
    TRY(get_stream(&st));
    DevBuf d_alc, d_rgb;
    StreamDrain drain(st);
    TRY(d_alc.alloc(len));
    TRY(d_rgb.alloc(bytes));
    for (const PartialSpan& s : spans)
        if (s.len) HIP_TRY(hipMemcpyAsync(d_alc.as<uint8_t>() + s.off, data + s.off, s.len, hipMemcpyHostToDevice, st));
    TRY(device(d_alc.as<uint8_t>(), d_rgb.p, st, payload_bytes));
    TRY(copy_to_host(out.get(), d_rgb.p, bytes, st));
    *out_len = bytes;
    *result = out.release();
    return kOk;
}

// The device calls: the null checks, the header read back and validated with the range, then decode(h, d, stream).  Nothing
// is queued before the header and the range have been accepted.
template <typename Decode>
int band_partial_decode_dev(const void* d_alc, uint64_t len, uint32_t first, uint32_t count, const void* d_rgb_out, void* hip_stream, Decode decode) {
    clear_error();
    if (!d_alc || !d_rgb_out) return fail(kNullArgument, "null argument");
    TRY(ensure_device());
    hipStream_t st = (hipStream_t)hip_stream;
    ScopeStream scope(st);
    std::vector<uint8_t> raw(kBandHeaderBytes, 0);
    if (len) {
        HIP_TRY(hipMemcpyAsync(raw.data(), d_alc, std::min<uint64_t>(len, kBandHeaderBytes), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    BandHeader h;
    ChunkDims d{};
    TRY(band_partial_validate(raw.data(), len, first, count, h, d));
    return decode(h, d, st);
}

}  // namespace

extern "C" {

int alice_codec_dev_decode_banded_frames(const void* d_alc, uint64_t len, uint32_t first, uint32_t count, void* d_rgb_out, void* hip_stream) {
    return band_partial_decode_dev(d_alc, len, first, count, d_rgb_out, hip_stream, [&](const BandHeader& h, const ChunkDims& d, hipStream_t st) {
        return band_frames_decode_device(h, d, band_partial_plan(kBandFrames, h, d, first, count), (const uint8_t*)d_alc, first, count,
                                         RgbLayout{(uint8_t*)d_rgb_out, 3ull * h.width, 3ull * h.width * h.height}, st, 0);
    });
}

uint8_t* alice_codec_decode_banded_frames(const uint8_t* data, uint64_t len, uint32_t first, uint32_t count, uint64_t* out_len) {
    clear_error();
    if (!data || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    BandHeader h;
    ChunkDims d{};
    if (band_partial_validate(data, len, first, count, h, d) != kOk) return nullptr;
    const BandPartialPlan p = band_partial_plan(kBandFrames, h, d, first, count);
    uint8_t* out = nullptr;
    band_partial_decode_host(data, len, h, p, (uint64_t)h.width * h.height * count * 3, &out, out_len,
                             [&](const uint8_t* d_alc, void* d_rgb, hipStream_t st, uint64_t uploaded) {
                                 return band_frames_decode_device(h, d, p, d_alc, first, count,
                                                                  RgbLayout{(uint8_t*)d_rgb, 3ull * h.width, 3ull * h.width * h.height}, st, uploaded);
                             });
    return out;
}

int alice_codec_dev_decode_banded_preview(const void* d_alc, uint64_t len, uint32_t first, uint32_t count, void* d_rgb_out, void* hip_stream) {
    return band_partial_decode_dev(d_alc, len, first, count, d_rgb_out, hip_stream, [&](const BandHeader& h, const ChunkDims& d, hipStream_t st) {
        return band_preview_decode_device(h, d, band_partial_plan(kBandPreview, h, d, first, count), (const uint8_t*)d_alc, first, count,
                                          d_rgb_out, st, 0);
    });
}

uint8_t* alice_codec_decode_banded_preview(const uint8_t* data, uint64_t len, uint32_t first, uint32_t count, uint64_t* out_len) {
    clear_error();
    if (!data || !out_len) { fail(kNullArgument, "null argument"); return nullptr; }
    BandHeader h;
    ChunkDims d{};
    if (band_partial_validate(data, len, first, count, h, d) != kOk) return nullptr;
    const BandPartialPlan p = band_partial_plan(kBandPreview, h, d, first, count);
    uint8_t* out = nullptr;
    band_partial_decode_host(data, len, h, p, (d.pw / 2) * (d.ph / 2) * count * 3, &out, out_len,
                             [&](const uint8_t* d_alc, void* d_rgb, hipStream_t st, uint64_t uploaded) {
                                 return band_preview_decode_device(h, d, p, d_alc, first, count, d_rgb, st, uploaded);
                             });
    return out;
}

void alice_codec_test_last_banded_frames_stats(uint64_t out[6]) {
    const BandPartialStats& s = tl_band_partial_stats[kBandFrames];
    const uint64_t v[6] = {s.a, s.b, s.blocks, s.uploaded, s.frames, s.stored};
    if (out) memcpy(out, v, sizeof(v));
}

void alice_codec_test_last_banded_preview_stats(uint64_t out[6]) {
    const BandPartialStats& s = tl_band_partial_stats[kBandPreview];
    const uint64_t v[6] = {s.a, s.b, s.blocks, s.uploaded, s.frames, s.stored};
    if (out) memcpy(out, v, sizeof(v));
}

}  // extern "C"
