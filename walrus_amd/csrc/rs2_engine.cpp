// Host side of the MI355X Red Stuff engine: the device runtime, the launch of planned codec
// jobs, blob plans and the C ABI declared in include/walrus_rs2.h.  The GF(2^16) constant tables
// and the codec job planner are rs2_planner.cpp, which touches no device.
//
// Reference semantics (paths relative to the reference checkout):
//   encoding/blob_encoding.rs:277-368  encode_with_metadata    -> rs2_encode_device_async
//   encoding/blob_encoding.rs:888-993  BlobDecoder::decode      -> rs2_decode_device_async
//   encoding/basic_encoding.rs:107-429 ReedSolomonEncoder/Decoder -> rs2_encode_1d / rs2_decode_1d
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <map>
#include <set>
#include <tuple>
#include <memory>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../../include/walrus_rs2.h"
#include "rs2_device.h"
#include "rs2_kernels.h"
#include "rs2_planner.h"

namespace rs2 {
namespace {

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(RS2_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));    \
  } while (0)

// Diagnostic: RS2_HOST_TRACE=<path> appends one "name ms" line per host-timed section (the
// decode's per-pattern setup), so the cost of individual calls can be read, not only the mean.
void host_trace(const char* name, double ms) {
  static FILE* f = [] {
    const char* e = std::getenv("RS2_HOST_TRACE");
    return e ? std::fopen(e, "a") : nullptr;
  }();
  if (!f) return;
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  std::fprintf(f, "%s %.4f\n", name, ms);
  std::fflush(f);
}

// ---------------------------------------------------------------------------------------------
// device context: per-device constant tables and a cache of transform table streams
// ---------------------------------------------------------------------------------------------
// Device memory arena, one per device: every DevBuf of plans, codecs, verifiers and contexts is
// a range of a few large hipMalloc'd segments (best fit over the free ranges, 256-byte
// granularity, neighbours coalesced on release), so plans created and destroyed for every new
// blob length -- the reference builds an encoder per call (config.rs:545-567) -- reuse device
// memory instead of calling hipMalloc / hipFree.  A segment is added only when no free range
// fits: max(request, reserved / 2, 256 MiB) rounded to 64 MiB, so the reserve grows
// geometrically and stops once it covers the workload's peak.  RS2_ARENA_RESERVE_MIB reserves
// a first segment up front (a hard budget: peak device memory = that reserve as long as the
// live buffers fit).  A range released by an owner that has quiesced its streams first (plan /
// codec / verifier destroy) is free at once; one released while work may still read it (a
// buffer outgrowing itself) waits in quarantine until a miss synchronizes the device.  Fully
// free segments beyond RS2_ARENA_CACHE_MIB of reserve (default 8192: the 256 MiB workload's
// double-buffered plans fit, a transient 4 GiB blob's do not stay) go back to hipFree, and
// rs2_device_memory_trim hands every wholly free segment back on request.
thread_local bool t_quiesced = false;  // the releasing owner has drained its streams

// For its scope the calling thread's releases count as quiesced: the owner has drained every
// stream and event its buffers' work ran behind, so their ranges are free at once.
struct Quiesced {
  const bool prev = t_quiesced;
  Quiesced() { t_quiesced = true; }
  ~Quiesced() { t_quiesced = prev; }
  Quiesced(const Quiesced&) = delete;
  Quiesced& operator=(const Quiesced&) = delete;
};

struct DevArena {
  static constexpr size_t kGrain = 256;
  struct Seg {
    uint8_t* base;
    size_t size;
    size_t used = 0;
    std::map<size_t, size_t> free_;  // offset -> length
  };
  std::mutex mu;
  std::vector<std::unique_ptr<Seg>> segs;
  std::set<std::tuple<size_t, size_t, size_t>> by_size;  // (length, segment, offset)
  std::vector<std::pair<void*, size_t>> quarantine_;
  size_t reserved = 0;
  uint64_t mallocs = 0, frees = 0, syncs = 0;
  int64_t live = 0, peak = 0;

  static size_t env_mib(const char* name, size_t dflt) {
    const char* e = std::getenv(name);
    return size_t(e ? std::max(0, std::atoi(e)) : int(dflt)) << 20;
  }
  static size_t cap() {
    static const size_t c = env_mib("RS2_ARENA_CACHE_MIB", 8192);
    return c;
  }
  size_t seg_of(const void* p) const {
    for (size_t k = 0; k < segs.size(); ++k)
      if (segs[k] && p >= segs[k]->base && p < segs[k]->base + segs[k]->size) return k;
    return SIZE_MAX;
  }
  void add_free(size_t k, size_t off, size_t len) {  // coalesces with both neighbours
    Seg& sg = *segs[k];
    auto nx = sg.free_.lower_bound(off);
    if (nx != sg.free_.end() && off + len == nx->first) {
      by_size.erase({nx->second, k, nx->first});
      len += nx->second;
      nx = sg.free_.erase(nx);
    }
    if (nx != sg.free_.begin()) {
      auto pv = std::prev(nx);
      if (pv->first + pv->second == off) {
        by_size.erase({pv->second, k, pv->first});
        off = pv->first;
        len += pv->second;
        sg.free_.erase(pv);
      }
    }
    sg.free_[off] = len;
    by_size.insert({len, k, off});
  }
  bool carve(size_t c, void** out) {
    auto it = by_size.lower_bound({c, 0, 0});
    if (it == by_size.end()) return false;
    const auto [len, k, off] = *it;
    by_size.erase(it);
    Seg& sg = *segs[k];
    sg.free_.erase(off);
    if (len > c) {
      sg.free_[off + c] = len - c;
      by_size.insert({len - c, k, off + c});
    }
    sg.used += c;
    *out = sg.base + off;
    return true;
  }
  hipError_t grow(size_t want) {
    uint8_t* p = nullptr;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), want);
    if (e != hipSuccess) return e;
    ++mallocs;
    size_t k = 0;
    while (k < segs.size() && segs[k]) ++k;
    if (k == segs.size()) segs.emplace_back();
    segs[k].reset(new Seg{p, want});
    reserved += want;
    add_free(k, 0, want);
    return hipSuccess;
  }
  hipError_t get(size_t n, void** out, size_t* got) {
    const size_t c = (std::max<size_t>(n, 1) + kGrain - 1) / kGrain * kGrain;
    std::unique_lock<std::mutex> lk(mu);
    if (reserved == 0) {
      static const size_t first = env_mib("RS2_ARENA_RESERVE_MIB", 0);
      if (first) {
        const hipError_t e = grow((first + (size_t(64) << 20) - 1) >> 26 << 26);
        if (e != hipSuccess) return e;
      }
    }
    bool ok = carve(c, out);
    if (!ok && !quarantine_.empty()) {
      // only the ranges quarantined before the synchronize are safe to release after it: take
      // them now, so a range another thread quarantines meanwhile stays quarantined
      std::vector<std::pair<void*, size_t>> q;
      q.swap(quarantine_);
      lk.unlock();
      const hipError_t e = hipDeviceSynchronize();
      lk.lock();
      if (e != hipSuccess) {
        quarantine_.insert(quarantine_.end(), q.begin(), q.end());
        return e;
      }
      ++syncs;
      std::vector<std::pair<void*, size_t>> to_free;  // segments past the cap
      for (auto& b : q) release_locked(b.first, b.second, &to_free);
      if (!to_free.empty()) {  // their hipFree outside the lock
        lk.unlock();
        for (auto& f : to_free) (void)hipFree(f.first);
        lk.lock();
      }
      ok = carve(c, out);
    }
    if (!ok) {
      size_t want = std::max({c, reserved / 2, size_t(256) << 20});
      want = (want + (size_t(64) << 20) - 1) >> 26 << 26;
      hipError_t e = grow(want);
      if (e != hipSuccess && want > c) e = grow((c + (size_t(2) << 20) - 1) >> 21 << 21);
      if (e != hipSuccess) return e;
      ok = carve(c, out);
      if (!ok) return hipErrorOutOfMemory;
    }
    live += int64_t(c);
    peak = std::max(peak, live);
    *got = c;
    return hipSuccess;
  }
  // Return a range to its segment.  A segment that falls wholly free past the cap leaves the
  // arena here, but its hipFree (which synchronizes the device) is the caller's, after the lock
  // is released, so other threads' allocations do not wait behind it.
  void release_locked(void* p, size_t c, std::vector<std::pair<void*, size_t>>* to_free) {
    const size_t k = seg_of(p);
    if (k == SIZE_MAX) return;
    Seg& sg = *segs[k];
    add_free(k, size_t(static_cast<uint8_t*>(p) - sg.base), c);
    sg.used -= c;
    if (sg.used == 0 && reserved > cap()) {  // trim a wholly free segment past the cap
      by_size.erase({sg.size, k, 0});
      reserved -= sg.size;
      ++frees;
      to_free->push_back({sg.base, sg.size});
      segs[k].reset();
    }
  }
  void put(void* p, size_t c, bool quiesced) {
    std::vector<std::pair<void*, size_t>> to_free;
    {
      std::lock_guard<std::mutex> lk(mu);
      live -= int64_t(c);
      if (quiesced)
        release_locked(p, c, &to_free);
      else
        quarantine_.push_back({p, c});
    }
    for (auto& f : to_free) (void)hipFree(f.first);
  }
  // every wholly free segment back to hipFree (quarantined ranges first released after a device
  // synchronize); returns the bytes handed back
  hipError_t trim(uint64_t* released) {
    std::unique_lock<std::mutex> lk(mu);
    std::vector<std::pair<void*, size_t>> to_free;
    if (!quarantine_.empty()) {
      std::vector<std::pair<void*, size_t>> q;  // snapshot before the synchronize (see get)
      q.swap(quarantine_);
      lk.unlock();
      const hipError_t e = hipDeviceSynchronize();
      lk.lock();
      if (e != hipSuccess) {
        quarantine_.insert(quarantine_.end(), q.begin(), q.end());
        return e;
      }
      ++syncs;
      for (auto& b : q) release_locked(b.first, b.second, &to_free);
    }
    uint64_t got = 0;
    for (auto& f : to_free) got += f.second;  // past the cap while leaving quarantine
    for (size_t k = 0; k < segs.size(); ++k) {
      if (!segs[k] || segs[k]->used) continue;
      Seg& sg = *segs[k];
      by_size.erase({sg.size, k, 0});
      reserved -= sg.size;
      got += sg.size;
      ++frees;
      to_free.push_back({sg.base, sg.size});
      segs[k].reset();
    }
    lk.unlock();
    for (auto& f : to_free) (void)hipFree(f.first);
    if (released) *released = got;
    return hipSuccess;
  }
};

DevArena& dev_arena(int device) {
  // never destroyed: buffers of objects torn down at process exit (the contexts) still return here
  static DevArena* arenas = new DevArena[64];
  return arenas[std::min(std::max(device, 0), 63)];
}

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;  // usable bytes (the arena range is bytes + 256, a multiple of 256)
  size_t cls = 0;
  int dev = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) dev_arena(dev).put(p, cls, t_quiesced);
    p = nullptr;
    bytes = 0;
    cls = 0;
  }
  hipError_t ensure(size_t n) {
    if (bytes >= n && p) return hipSuccess;
    release();
    // 256 bytes of slack: kernels may read whole dwords past a symbol's last byte
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    size_t got = 0;
    e = dev_arena(dev).get(n + 256, &p, &got);
    if (e == hipSuccess) {
      bytes = got - 256;
      cls = got;
    } else {
      p = nullptr;
    }
    return e;
  }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

std::atomic<uint64_t> g_pinned_allocs{0};

struct PinnedBuf {
  void* p = nullptr;
  size_t bytes = 0;
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
  hipError_t ensure(size_t n) {
    if (bytes >= n && p) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
    hipError_t e = hipHostMalloc(&p, n, hipHostMallocDefault);
    if (e == hipSuccess) {
      bytes = n;
      g_pinned_allocs.fetch_add(1, std::memory_order_relaxed);
    }
    return e;
  }
};

// A timing-disabled event, created on first use.  Unset it orders nothing: wait_on and sync
// return at once.  Destroying it waits for nothing.
struct Event {
  hipEvent_t ev = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() {
    if (ev) (void)hipEventDestroy(ev);
  }
  bool set() const { return ev != nullptr; }
  hipError_t record(hipStream_t st) {
    if (!ev) {
      const hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
      if (e != hipSuccess) return e;
    }
    return hipEventRecord(ev, st);
  }
  hipError_t wait_on(hipStream_t st) const { return ev ? hipStreamWaitEvent(st, ev, 0) : hipSuccess; }
  hipError_t sync() const { return ev ? hipEventSynchronize(ev) : hipSuccess; }
};

// Host worker threads for the pinned staging of the host-buffer ABI: copies between the
// caller's pageable buffers and pinned slots run on several cores while the DMA engine moves
// the previous slot (one core's memcpy would cap the path at ~10 GB/s).  Shared by every plan
// of a device; run() is re-entrant (each call waits only for its own tasks).
class HostPool {
 public:
  ~HostPool() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  int threads() {
    start();
    return int(th_.size()) + 1;
  }
  // Run every task (the calling thread takes a share) and return when all have finished.
  void run(std::vector<std::function<void()>>& tasks) {
    start();
    if (tasks.empty()) return;
    struct Latch {
      std::mutex m;
      std::condition_variable cv;
      size_t left;
    };
    auto latch = std::make_shared<Latch>();
    latch->left = tasks.size();
    auto finish = [latch]() {
      std::lock_guard<std::mutex> lk(latch->m);
      if (--latch->left == 0) latch->cv.notify_all();
    };
    {
      std::lock_guard<std::mutex> lk(mu_);
      for (size_t i = 1; i < tasks.size(); ++i) {
        std::function<void()> t = std::move(tasks[i]);
        q_.emplace_back([t, finish]() {
          t();
          finish();
        });
      }
    }
    cv_.notify_all();
    tasks[0]();
    finish();
    std::unique_lock<std::mutex> lk(latch->m);
    latch->cv.wait(lk, [&] { return latch->left == 0; });
  }

 private:
  void start() {
    std::call_once(once_, [this] {
      int n = int(std::thread::hardware_concurrency());
      int want = env_int("RS2_HOST_THREADS", 16);
      want = std::max(1, std::min(want, std::max(n, 1)));
      for (int i = 0; i + 1 < want; ++i) th_.emplace_back([this] { loop(); });
    });
  }
  void loop() {
    for (;;) {
      std::function<void()> t;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
        if (stop_ && q_.empty()) return;
        t = std::move(q_.front());
        q_.pop_front();
      }
      t();
    }
  }
  std::once_flag once_;
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::function<void()>> q_;
  bool stop_ = false;
};

// One piece of a host <-> device transfer: `len` bytes between host `h` and device `d`.
struct Seg {
  uint8_t* h;
  uint8_t* d;
  size_t len;
};

// memcpy of many segments split evenly over the pool's threads (dst/src per direction)
void par_copy(HostPool& pool, const std::vector<Seg>& segs, bool to_host) {
  size_t total = 0;
  for (const auto& g : segs) total += g.len;
  if (total == 0) return;
  const int T = int(std::min<size_t>(size_t(pool.threads()), (total + (1 << 20) - 1) >> 20));
  const size_t per = (total + T - 1) / T;
  std::vector<std::vector<Seg>> parts(T);
  size_t acc = 0;
  for (const auto& g : segs) {
    size_t off = 0;
    while (off < g.len) {
      const int t = int(std::min<size_t>(acc / per, size_t(T - 1)));
      const size_t room = (size_t(t) + 1) * per - acc;
      const size_t take = std::min(g.len - off, t == T - 1 ? g.len - off : room);
      parts[t].push_back({g.h + off, g.d + off, take});
      off += take;
      acc += take;
    }
  }
  std::vector<std::function<void()>> tasks;
  for (auto& part : parts) {
    if (part.empty()) continue;
    tasks.emplace_back([&part, to_host] {
      for (const auto& g : part) {
        if (to_host)
          std::memcpy(g.h, g.d, g.len);
        else
          std::memcpy(g.d, g.h, g.len);
      }
    });
  }
  pool.run(tasks);
}

// fn(i) for every i < cnt, strided over the pool's threads
template <class F>
void pool_for_each(HostPool& pool, size_t cnt, F fn) {
  if (!cnt) return;
  const size_t T = std::min<size_t>(size_t(pool.threads()), cnt);
  std::vector<std::function<void()>> tasks;
  for (size_t t = 0; t < T; ++t)
    tasks.emplace_back([&fn, t, T, cnt] {
      for (size_t i = t; i < cnt; i += T) fn(i);
    });
  pool.run(tasks);
}

// Pinned slots for the small per-call uploads (a decode's position offsets, mixing tables and
// multiplier logs, copy lists, verifier targets).  A hipMemcpyAsync host -> device on a stream
// that has kernels queued can block the issuing thread until they have run (the copy engine's
// dependency on the compute queue): the bench's timed decodes 4 and 6 stalled 6-7 ms each that
// way in every run, whatever its length, from pageable sources (gpurun_out/r05a traces: the
// 0.6 ms per step the 20-step driver run showed as dec_plan_host) and 15-28 ms from pinned ones
// (gpurun_out/r05c).  So the data goes into a pinned, device-mapped slot and a copy kernel
// (rs2_copy.hip host_upload_kernel) moves it in stream order like any other launch.  kSlots
// slots of kSlotBytes, pinned once per device at first use and never grown; uploads take them
// round-robin.
//
// Reuse of a slot.  Every use of slot k carries a generation number; the kernel that last reads
// the slot stores that generation into word k of a coherent, device-mapped host array when it
// has finished (rs2_copy.hip host_upload_kernel / upload_signal_kernel),
// and the host rewrites the slot only once it reads that generation there.  No HIP event is
// involved, so the wait depends on nothing but the copy having run -- not on the stream it ran
// on still existing (plans, verifiers and caller streams come and go between uploads; an event
// recorded on a destroyed stream is refused by the runtime) -- and it never waits for more than
// that one copy (no device-wide synchronize).  With 64 slots the wait is reached only with 64
// uploads still queued (rs2_upload_stats counts the waits).  Both rings are allocated coherent
// (fine-grained), so the copy kernel's reads of a rewritten slot never depend on GPU cache state.
// Larger uploads (n_shards in the thousands) keep the runtime's path.
std::atomic<uint64_t> g_upload_calls{0}, g_upload_waits{0}, g_upload_jobs{0};

class UploadSlots {
 public:
  static constexpr int kSlots = 64;
  static constexpr size_t kSlotBytes = size_t(512) << 10;
  // (lives as long as its Context, i.e. to process exit: the pinned blocks are left to the process
  // teardown rather than freed while the runtime may already be going down)
  hipError_t upload(void* dst, const void* src, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (n > kSlotBytes) return hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st);
    std::lock_guard<std::mutex> lk(mu_);
    hipError_t e = init_locked();
    if (e != hipSuccess) return e;
    if (!base_) {
      e = pin(&base_, &dev_base_, kSlots * kSlotBytes);
      if (e != hipSuccess) return e;
    }
    const int k = next_;
    next_ = (next_ + 1) % kSlots;
    if ((e = wait_locked(k)) != hipSuccess) return e;
    uint8_t* slot = base_ + size_t(k) * kSlotBytes;
    std::memcpy(slot, src, n);
    const uint64_t g = ++gen_counter_;
    // a copy kernel reading the mapped slot, not hipMemcpyAsync (rs2_copy.hip host_upload_kernel);
    // its one workgroup reports generation g in word k once every load of the slot has returned
    e = rs2k_launch_host_upload(dev_base_ + size_t(k) * kSlotBytes, dst, int64_t(n),
                                done_dev_ + k, g, st);
    if (e != hipSuccess) return e;  // not launched: the slot stays free (want_ unchanged)
    want_[k] = g;
    g_upload_calls.fetch_add(1, std::memory_order_relaxed);
    return hipSuccess;
  }

  // A CodecJobBig for one launch: staged into a pinned slot, copied by the copy kernel into a
  // device slot of its own, `launch(device pointer)` enqueues the consumer on st, and a signal
  // kernel queued behind the consumer reports the slot pair free.  (Jobs of more than kMaxBlocks
  // blocks: n_shards above about 24,580.)
  template <class F>
  hipError_t launch_with_job(const void* src, size_t n, hipStream_t st, F launch) {
    if (n > kSlotBytes) return hipErrorInvalidValue;
    std::lock_guard<std::mutex> lk(mu_);
    hipError_t e = init_locked();
    if (e != hipSuccess) return e;
    if (!jbase_) {
      if ((e = pin(&jbase_, &jdev_host_, kJobSlots * kSlotBytes)) != hipSuccess) return e;
      if ((e = jdev_.ensure(kJobSlots * kSlotBytes)) != hipSuccess) return e;
    }
    const int k = jnext_;
    jnext_ = (jnext_ + 1) % kJobSlots;
    const int w = kSlots + k;  // completion word of job slot k
    if ((e = wait_locked(w)) != hipSuccess) return e;
    std::memcpy(jbase_ + size_t(k) * kSlotBytes, src, n);
    uint8_t* d = jdev_.as<uint8_t>() + size_t(k) * kSlotBytes;
    const uint64_t g = ++gen_counter_;
    e = rs2k_launch_host_upload(jdev_host_ + size_t(k) * kSlotBytes, d, int64_t(n), nullptr, 0,
                                st);
    if (e != hipSuccess) return e;
    const hipError_t le = launch(d);
    // reported whether or not the consumer launched: the copy above did, and reads the slot
    e = rs2k_launch_upload_signal(done_dev_ + w, g, st);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(st);  // no report coming: the copy (and consumer) have run
      return le != hipSuccess ? le : e;
    }
    want_[w] = g;
    g_upload_jobs.fetch_add(1, std::memory_order_relaxed);
    return le;
  }

 private:
  static constexpr int kJobSlots = 16;
  static constexpr int kWords = kSlots + kJobSlots;
  static hipError_t pin(uint8_t** host, uint8_t** dev, size_t bytes) {
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) return e;
    g_pinned_allocs.fetch_add(1, std::memory_order_relaxed);
    void* dp = nullptr;
    if ((e = hipHostGetDevicePointer(&dp, p, 0)) != hipSuccess) return e;
    *host = static_cast<uint8_t*>(p);
    *dev = static_cast<uint8_t*>(dp);
    return hipSuccess;
  }
  // the completion words (coherent host memory, device-mapped)
  hipError_t init_locked() {
    if (done_host_) return hipSuccess;
    uint8_t *h = nullptr, *d = nullptr;
    hipError_t e = pin(&h, &d, kWords * sizeof(uint64_t));
    if (e != hipSuccess) return e;
    std::memset(h, 0, kWords * sizeof(uint64_t));
    done_host_ = reinterpret_cast<uint64_t*>(h);
    done_dev_ = reinterpret_cast<uint64_t*>(d);
    return hipSuccess;
  }
  // Wait (spinning, then yielding) until word w reports the generation its slot was last used
  // with.  A copy that never runs (a faulted device) ends the wait with an error after 120 s.
  hipError_t wait_locked(int w) {
    const uint64_t want = want_[w];
    if (want == 0 || __atomic_load_n(done_host_ + w, __ATOMIC_ACQUIRE) >= want) return hipSuccess;
    g_upload_waits.fetch_add(1, std::memory_order_relaxed);
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t spin = 0; __atomic_load_n(done_host_ + w, __ATOMIC_ACQUIRE) < want; ++spin) {
      if (spin < 4096) continue;
      std::this_thread::yield();
      if ((spin & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120))
        return hipErrorLaunchTimeOut;
    }
    return hipSuccess;
  }
  std::mutex mu_;
  uint64_t* done_host_ = nullptr;  // [kWords] completion words as the host reads them
  uint64_t* done_dev_ = nullptr;   // the same words as the device addresses them
  uint64_t gen_counter_ = 0;
  uint64_t want_[kWords] = {};     // generation of each slot's last use (0 = never used)
  uint8_t* base_ = nullptr;
  uint8_t* dev_base_ = nullptr;    // the same slots as the device addresses them
  int next_ = 0;
  uint8_t* jbase_ = nullptr;
  uint8_t* jdev_host_ = nullptr;
  DevBuf jdev_;
  int jnext_ = 0;
};

struct Dec1D;  // rs2_decode_1d's pooled state (below)

struct Context {
  int device = 0;
  HostPool pool;
  DevBuf exp_t, log_t;
  std::mutex mu;
  std::map<std::tuple<int, int, int>, std::unique_ptr<DevBuf>> streams;
  hipStream_t util_stream = nullptr;
  UploadSlots uploads;
  hipError_t upload(void* dst, const void* src, size_t n, hipStream_t st) {
    return uploads.upload(dst, src, n, st);
  }
  // Pooled helpers of the host-buffer single-sliver entry points (SliverData::verify /
  // get_merkle_root, recovery symbols, the 1D decode of a sliver recovery): a storage node calls
  // them one sliver at a time, so a verifier (stream, encode plan, device buffers, pinned
  // staging) or a 1D decoder is checked out of a pool per parameter set instead of being built
  // and torn down per call (a fresh stream and plan cost more than the work at n = 1000).
  std::mutex pool_mu;
  std::map<std::tuple<int, int, int>, std::vector<::rs2_verifier*>> verifier_pool;
  std::map<std::tuple<int, int, int>, std::vector<Dec1D*>> dec1d_pool;
  std::map<int, std::vector<::rs2_sliver_checker*>> checker_pool;  // rs2_verify_slivers_mixed, by n_shards
  static constexpr size_t kPoolKeep = 8;  // idle objects kept per parameter set

  int init(int dev) {
    device = dev;
    HIP_TRY(hipSetDevice(dev));
    const Gf& g = gf();
    HIP_TRY(exp_t.ensure(kOrder * 2));
    HIP_TRY(log_t.ensure(kOrder * 2));
    HIP_TRY(hipMemcpy(exp_t.p, g.exp.data(), kOrder * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(log_t.p, g.log.data(), kOrder * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipStreamCreateWithFlags(&util_stream, hipStreamNonBlocking));
    return RS2_OK;
  }

  // device table stream for a size-C transform with skew offset sd, laid out for `ppw`
  // positions per wave (built once, cached)
  const uint16_t* stream(int C, int sd, int ppw) {
    std::lock_guard<std::mutex> lk(mu);
    auto key = std::make_tuple(C, sd, ppw);
    auto it = streams.find(key);
    if (it != streams.end()) return it->second->as<uint16_t>();
    std::vector<uint16_t> host = sd_stream(C, sd, ppw);
    auto buf = std::make_unique<DevBuf>();
    if (buf->ensure(std::max<size_t>(host.size() * 2, 16)) != hipSuccess) return nullptr;
    if (!host.empty() &&
        hipMemcpy(buf->p, host.data(), host.size() * 2, hipMemcpyHostToDevice) != hipSuccess)
      return nullptr;
    const uint16_t* p = buf->as<uint16_t>();
    streams.emplace(key, std::move(buf));
    return p;
  }
};

std::mutex g_ctx_mu;
std::map<int, std::unique_ptr<Context>> g_ctx;
thread_local int g_device = 0;

int get_context(Context** out) {
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  auto it = g_ctx.find(g_device);
  if (it != g_ctx.end()) {
    *out = it->second.get();
    return hipSetDevice(g_device) == hipSuccess ? RS2_OK : fail(RS2_E_DEVICE, "hipSetDevice");
  }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= g_device)
    return fail(RS2_E_DEVICE, "no HIP device available");
  auto ctx = std::make_unique<Context>();
  RS2_TRY(ctx->init(g_device));
  *out = ctx.get();
  g_ctx.emplace(g_device, std::move(ctx));
  return RS2_OK;
}

// Diagnostic phase stamps (a library built with -DRS2_STAMPS=1 and $RS2_STAMP_FILE set): every
// codec launch runs synchronously and appends {mode, C, tiles, n_z, kStamps, waves} + the stamps
// of every wave of every workgroup to the file (tools/stamps_summary.py reads it).
hipError_t stamp_dump(int C, int mode, int tiles, int n_z, uint64_t* d, hipStream_t st) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  hipError_t e = hipStreamSynchronize(st);
  if (e != hipSuccess) return e;
  const int nw = std::max(1, C / kPpwTarget);
  std::vector<uint64_t> h(size_t(tiles) * n_z * nw * kStamps);
  e = hipMemcpy(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return e;
  if (FILE* f = std::fopen(std::getenv("RS2_STAMP_FILE"), "ab")) {
    const int32_t hdr[6] = {mode, C, tiles, n_z, kStamps, nw};
    std::fwrite(hdr, sizeof hdr, 1, f);
    std::fwrite(h.data(), 8, h.size(), f);
    std::fclose(f);
  }
  return hipSuccess;
}

// n_blobs > 1: the same job over a batch of blobs whose symbols lie in_bs / out_bs / cp_bs
// bytes apart (CodecJob::tiles_per_blob); the grid holds every blob's tiles.
// tile_ctr: kTileCtrWords zeroed words owned by this launch site (CodecJob::tile_ctr), used when
// the job runs as a pipelined kernel and RS2_PIPE_DYN=1; null = static tile ranges.
// The job as the kernels' by-value argument: every scalar field at once (CodecScalars), the
// block arrays and mixing kinds cut to kMaxBlocks (the caller checked that n_in, n_out <=
// kMaxBlocks); rs2_device.h static_asserts that the arrays listed here are all there is.
void narrow_job(const CodecJobBig& b, CodecJob& s) {
  static_cast<CodecScalars&>(s) = static_cast<const CodecScalars&>(b);
  std::copy(b.in, b.in + kMaxBlocks, s.in);
  std::copy(b.out, b.out + kMaxBlocks, s.out);
  for (int o = 0; o < kMaxBlocks; ++o) {
    std::memcpy(s.m1_kind[o], b.m1_kind[o], kMaxBlocks);
    std::memcpy(s.m2_kind[o], b.m2_kind[o], kMaxBlocks);
  }
  std::copy(b.pair_p, b.pair_p + kMaxBlocks, s.pair_p);
  std::copy(b.pair_q, b.pair_q + kMaxBlocks, s.pair_q);
  std::copy(b.pair_nw, b.pair_nw + kMaxBlocks, s.pair_nw);
}

// CUs of the current device (0 when it cannot be read)
int cu_count() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  return cus;
}

// The per-launch fields of a job over n_blobs blobs: the lines (folded into grid.x with the
// element pairs) and the blobs' strides.  Returns the launch's tiles, or -1 when they do not
// fit a grid dimension.
int set_launch_shape(CodecScalars& job, int n_lines, int n_blobs, int64_t in_bs, int64_t out_bs,
                     int64_t cp_bs) {
  job.n_lines = n_lines;
  const int64_t per_blob = (int64_t(n_lines) * job.pairs_span + 63) / 64;
  const int64_t tiles64 = per_blob * n_blobs;
  if (tiles64 > 0x7FFFFFFF) return -1;
  job.tiles_per_blob = n_blobs > 1 ? int(per_blob) : 0;
  job.in_blob_stride = in_bs;
  job.out_blob_stride = out_bs;
  job.copy_blob_stride = cp_bs;
  job.stamps = nullptr;
  return int(tiles64);
}

// A job of more than kMaxBlocks blocks (C = 512): one-tile kernels reading the job from device
// memory (no pipelined / persistent variants, no stamps).
hipError_t launch_codec_big(const CodecJobBig& job_in, int n_lines, int n_z, int mode,
                            hipStream_t st, int n_blobs, int64_t in_bs, int64_t out_bs,
                            int64_t cp_bs) {
  if (mode != kModeRows && mode != kModeCols && mode != kModeDecode) return hipErrorInvalidValue;
  auto job = std::make_unique<CodecJobBig>(job_in);
  const int tiles = set_launch_shape(*job, n_lines, n_blobs, in_bs, out_bs, cp_bs);
  if (tiles < 0) return hipErrorInvalidValue;
  job->tile_ctr = nullptr;
  Context* ctx = nullptr;
  if (get_context(&ctx) != RS2_OK) return hipErrorInvalidDevice;
  return ctx->uploads.launch_with_job(job.get(), sizeof(CodecJobBig), st, [&](uint8_t* d) {
    return rs2k_launch_codec_big_512(reinterpret_cast<const CodecJobBig*>(d), tiles, 1, n_z, mode,
                                     st);
  });
}

hipError_t launch_codec_c(int C, const CodecJobBig& job_big, int n_lines, int n_z, int mode,
                          hipStream_t st, int n_blobs = 1, int64_t in_bs = 0, int64_t out_bs = 0,
                          int64_t cp_bs = 0, uint32_t* tile_ctr = nullptr) {
  if (job_big.n_pairs <= 0 || n_lines <= 0 || job_big.pairs_span < job_big.n_pairs) return hipSuccess;
  if (n_blobs < 1) return hipErrorInvalidValue;
  if (job_big.n_in > kMaxBlocks || job_big.n_out > kMaxBlocks) {
    // more blocks than the kernel argument holds (n_shards above about 24,580)
    if (C != kMaxC) return hipErrorInvalidValue;
    return launch_codec_big(job_big, n_lines, n_z, mode, st, n_blobs, in_bs, out_bs, cp_bs);
  }
  CodecJob job;
  narrow_job(job_big, job);
  const int tiles = set_launch_shape(job, n_lines, n_blobs, in_bs, out_bs, cp_bs);
  if (tiles < 0) return hipErrorInvalidValue;
  n_lines = 1;  // lines are folded into grid.x
  // Shared-input jobs whose last output block's active waves fit below the input's run as the
  // persistent tile-pipelined kernel (rs2_codec.hip cols_pipe_body): one workgroup per CU, each
  // walking a contiguous tile range.  RS2_PIPE=0: never (A/B knob).
  int grid_tiles = tiles;
  if (((mode == kModeCols && job.shared_in && job.n_out <= 3) ||
       (mode == kModeRows && !job.shared_in && job.n_out == 1)) &&
      n_z == 1 && job.n_out >= 1 && C >= 2 * kPpwTarget) {
    static const int pipe_wgs = [] {
      const int k = env_int("RS2_PIPE", 1);  // RS2_PIPE=k: k workgroups per CU
      const int cus = k == 0 ? 0 : cu_count();
      if (cus == 0) return 0;
      const int wgs = env_int("RS2_PIPE_WGS", 0);  // A/B: an absolute workgroup count
      return wgs > 0 ? wgs : cus * std::max(1, k);
    }();
    const int nw = C / kPpwTarget;
    auto waves = [](int count) { return (count + kPpwTarget - 1) / kPpwTarget; };
    const int tail_waves = waves(job.out[job.n_out - 1].trunc);
    // the head input block: the shared input, or the mixing job's shortest block (every block
    // of a pipelined mixing job must carry a nonzero coefficient)
    int head = 0;
    bool ok = pipe_wgs > 0;
    if (mode == kModeRows)
      for (int b = 0; b < job.n_in && ok; ++b) {
        ok = job.m2_kind[0][b] != 0 && job.m1_kind[0][b] == 0;
        if (job.in[b].count < job.in[head].count) head = b;
      }
    if (ok && waves(job.in[head].count) + tail_waves <= nw) {
      mode = mode == kModeCols ? kModeColsPipe : kModeRowsPipe;
      job.n_tiles = tiles;
      job.pipe_head = head;
      grid_tiles = std::min(tiles, pipe_wgs);
      // RS2_PIPE_DYN=1: dynamic tile order (A/B knob; static ranges measured 82.5 vs 81.4 GiB/s,
      // and with a high-priority decode stream 63.0 vs 63.2: profiles/r03/exp/dyn/)
      static const bool dyn = env_int("RS2_PIPE_DYN", 0) != 0;
      job.tile_ctr = dyn ? tile_ctr : nullptr;
    }
  }
  // The decode as one persistent workgroup per CU (kModeDecodePersist) when RS2_DEC_PERSIST=k
  // (k workgroups per CU) is set: A/B knob
  if (mode == kModeDecode && n_z == 1) {
    static const int dec_wgs = [] {
      const int k = env_int("RS2_DEC_PERSIST", 0);
      return k > 0 ? cu_count() * k : 0;
    }();
    if (dec_wgs > 0 && tiles > dec_wgs) {
      mode = kModeDecodePersist;
      job.n_tiles = tiles;
      grid_tiles = dec_wgs;
    }
  }
  static const bool stamping = std::getenv("RS2_STAMP_FILE") != nullptr;
  if (stamping) {
    const size_t n_st = size_t(tiles) * n_z * std::max(1, C / kPpwTarget) * kStamps;
    hipError_t e = hipMalloc(&job.stamps, n_st * 8);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(job.stamps, 0, n_st * 8, st);
    if (e != hipSuccess) return e;
  }
  hipError_t le = hipSuccess;
  switch (C) {
    case 1: le = rs2k_launch_codec_1(&job, grid_tiles, n_lines, n_z, mode, st); break;
    case 2: le = rs2k_launch_codec_2(&job, grid_tiles, n_lines, n_z, mode, st); break;
    case 4: le = rs2k_launch_codec_4(&job, grid_tiles, n_lines, n_z, mode, st); break;
    case 8: le = rs2k_launch_codec_8(&job, grid_tiles, n_lines, n_z, mode, st); break;
    case 16: le = rs2k_launch_codec_16(&job, grid_tiles, n_lines, n_z, mode, st); break;
    case 32: le = rs2k_launch_codec_32(&job, grid_tiles, n_lines, n_z, mode, st); break;
    case 64: le = rs2k_launch_codec_64(&job, grid_tiles, n_lines, n_z, mode, st); break;
    case 128: le = rs2k_launch_codec_128(&job, grid_tiles, n_lines, n_z, mode, st); break;
    case 256: le = rs2k_launch_codec_256(&job, grid_tiles, n_lines, n_z, mode, st); break;
    case 512: le = rs2k_launch_codec_512(&job, grid_tiles, n_lines, n_z, mode, st); break;
    default: le = hipErrorInvalidValue;
  }
  if (le != hipSuccess || !stamping) return le;
  return stamp_dump(C, mode, grid_tiles, n_z, job.stamps, st);
}

// A planned job over n_lines lines of one blob (the lines are folded into grid.x with the element
// pairs, CodecJob::pairs_span).
hipError_t launch_job(const PlannedJob& pj, int n_lines, hipStream_t st,
                      uint32_t* tile_ctr = nullptr) {
  return launch_codec_c(pj.C, pj.job, n_lines, pj.n_z, pj.mode, st, 1, 0, 0, 0, tile_ctr);
}

// Device memory holding a planned job's arrays.
struct JobMem {
  DevBuf offs, pre_tab, post_tab, mix, logs;
};

// rs2_decode_1d's state per (k, n_shards, symbol size), pooled in the Context (a sliver
// recovery decodes one codeword of K symbols per call): its stream, device buffers, pinned
// staging and the planned decode job's device arrays.
struct Dec1D {
  hipStream_t st = nullptr;
  DevBuf din, dout;
  PinnedBuf hin, hout;
  PlannedJob pj;
  JobMem mem;
};

// checkout / return of a pooled Dec1D (returned with its stream drained: rs2_decode_1d
// synchronizes before it returns)
struct Dec1DLease {
  Context* ctx = nullptr;
  std::tuple<int, int, int> key;
  Dec1D* d = nullptr;
  Dec1DLease(Context* c, int k, int n, int s) : ctx(c), key(k, n, s) {}
  Dec1DLease(const Dec1DLease&) = delete;
  Dec1DLease& operator=(const Dec1DLease&) = delete;
  hipError_t get() {
    {
      std::lock_guard<std::mutex> lk(ctx->pool_mu);
      auto& free_ = ctx->dec1d_pool[key];
      if (!free_.empty()) {
        d = free_.back();
        free_.pop_back();
        return hipSuccess;
      }
    }
    auto nd = std::make_unique<Dec1D>();
    hipError_t e = hipStreamCreateWithFlags(&nd->st, hipStreamNonBlocking);
    if (e != hipSuccess) return e;
    d = nd.release();
    return hipSuccess;
  }
  ~Dec1DLease() {
    if (!d) return;
    // drained before it goes back: an error return may leave its H2D copy of hin (or the
    // decode) queued, and the next holder rewrites hin / grows it (PinnedBuf::ensure frees it)
    (void)hipStreamSynchronize(d->st);
    {
      std::lock_guard<std::mutex> lk(ctx->pool_mu);
      auto& free_ = ctx->dec1d_pool[key];
      if (free_.size() < Context::kPoolKeep) {
        free_.push_back(d);
        return;
      }
    }
    (void)hipStreamSynchronize(d->st);
    (void)hipStreamDestroy(d->st);
    const Quiesced quiesced;  // drained above: its ranges may be reused at once
    delete d;
  }
};

// Attach sd tables, upload the offsets and mixing tables.  Must follow plan_encode / plan_decode.
int bind_job(Context* ctx, PlannedJob& pj, JobMem& mem, hipStream_t st) {
  CodecJobBig& j = pj.job;
  const size_t n_off = finish_plan(pj);  // pairs_span; the copy offsets behind the positions
  auto t0 = std::chrono::steady_clock::now();
  auto lap = [&](const char* name) {
    const auto t1 = std::chrono::steady_clock::now();
    host_trace(name, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  };
  HIP_TRY(mem.offs.ensure(pj.offs.size() * 8));
  lap("bind_offs_ensure");
  HIP_TRY(ctx->upload(mem.offs.p, pj.offs.data(), pj.offs.size() * 8, st));
  lap("bind_offs_copy");
  for (int b = 0; b < j.n_in; ++b) {
    if (!pj.copy_offs.empty()) {
      j.in[b].copy_base = pj.copy_base;
      j.in[b].copy_off = mem.offs.as<int64_t>() + n_off + size_t(b) * pj.C;
      j.in[b].copy_line_stride = pj.copy_ls;
      j.in[b].copy_limit = pj.copy_limit;
    } else {
      j.in[b].copy_off = nullptr;
    }
    j.in[b].pos_off = mem.offs.as<int64_t>() + pj.in_off(b);
    j.in[b].sd_tab = ctx->stream(pj.C, pj.in_sd[b], pj.ppw);
    if (!j.in[b].sd_tab) return fail(RS2_E_DEVICE, "table upload failed");
    j.in[b].zero_first = group0_zero(pj.C, pj.in_sd[b], pj.ppw);
  }
  for (int o = 0; o < j.n_out; ++o) {
    j.out[o].pos_off = mem.offs.as<int64_t>() + pj.out_off(o);
    j.out[o].sd_tab = ctx->stream(pj.C, pj.out_sd[o], pj.ppw);
    if (!j.out[o].sd_tab) return fail(RS2_E_DEVICE, "table upload failed");
    j.out[o].zero_first = group0_zero(pj.C, pj.out_sd[o], pj.ppw);
  }
  lap("bind_sd_tables");
  if (pj.has_mix) {
    // the tables of output blocks o < n_out only (rows of mix_stride * 2 tables)
    const size_t used = std::min(pj.mix.size(), size_t(j.n_out) * pj.mix_stride * 2 * kTabU16);
    HIP_TRY(mem.mix.ensure(pj.mix.size() * 2));
    HIP_TRY(ctx->upload(mem.mix.p, pj.mix.data(), used * 2, st));
    j.mix_tab = mem.mix.as<uint16_t>();
    lap("bind_mix_copy");
  }
  return RS2_OK;
}

// Upload a decode job's arrays and build its per-position tables on the device.
int bind_decode(Context* ctx, PlannedJob& pj, JobMem& mem, hipStream_t st) {
  CodecJobBig& j = pj.job;
  RS2_TRY(bind_job(ctx, pj, mem, st));
  const size_t npre = pj.pre_logs.size(), npost = pj.post_logs.size();
  std::vector<uint16_t>& logs = pj.logs;
  logs.resize(npre + npost);
  std::copy(pj.pre_logs.begin(), pj.pre_logs.end(), logs.begin());
  std::copy(pj.post_logs.begin(), pj.post_logs.end(), logs.begin() + npre);
  HIP_TRY(mem.logs.ensure(std::max<size_t>(logs.size() * 2, 16)));
  HIP_TRY(mem.pre_tab.ensure(std::max<size_t>((npre + npost) * kTabU16 * 2, 16)));
  if (!logs.empty()) {
    HIP_TRY(ctx->upload(mem.logs.p, logs.data(), logs.size() * 2, st));
    HIP_TRY(rs2k_launch_build_mul_tables(ctx->exp_t.as<uint16_t>(), ctx->log_t.as<uint16_t>(),
                                         mem.logs.as<uint16_t>(), int(logs.size()),
                                         mem.pre_tab.as<uint16_t>(), st));
  }
  for (int b = 0; b < j.n_in; ++b)
    j.in[b].pre_tab = mem.pre_tab.as<uint16_t>() + size_t(b) * pj.C * kTabU16;
  j.pre_z_stride = int64_t(j.n_in) * pj.C * kTabU16;
  for (int o = 0; o < j.n_out; ++o)
    j.out[o].post_tab = mem.pre_tab.as<uint16_t>() + (npre + size_t(o) * pj.C) * kTabU16;
  return RS2_OK;
}

// One decode slot of a blob plan or a 1D codec.  Each holds two, taken in turn, so back-to-back
// async decodes never overwrite live arrays: a slot is rewritten only after `done`, the event
// of its last launch.
struct DecodeSlot {
  PlannedJob job;
  JobMem mem;
  // present originals copied outside the codec (when not fused into it): offsets on the device
  // and the host vectors they are uploaded from, alive until `done`
  DevBuf copy_src, copy_dst;
  std::vector<int64_t> copy_src_h, copy_dst_h;
  Event done;
  // the erasure pattern / buffers the slot's job was planned for: a repeat decode with the same
  // key reuses the slot's tables and offsets on the device instead of re-planning (empty: the
  // slot is never reused that way)
  std::vector<int64_t> key;
  bool fused = false;  // the job writes the present originals from its own loads
};

// One chunk of a decode batch: the concatenated position (and copy) offsets, multiplier logs,
// per-position tables, mixing tables and the job table of its blobs.  A plan holds two, taken
// in turn; a slot is rewritten only after `done`, the event of its last launch.
struct BatchDecodeSlot {
  DevBuf offs, logs, tabs, mix, jobs;
  Event done;
};
// Jobs of one chunk: what fits one upload slot; and the per-position tables of one chunk
// (256 bytes per multiplier log), so the device memory of a call does not grow with n_blobs.
constexpr size_t kBatchChunkJobs = UploadSlots::kSlotBytes / sizeof(CodecJobBatch);
constexpr size_t kBatchTableBytes = size_t(256) << 20;
std::atomic<uint64_t> g_batch_launches{0}, g_batch_blobs{0}, g_batch_single{0};

constexpr int kMerkleMaxLeaves = 4096;  // rs2_hash.hip kMerkleMax (one-wave / one-WG trees)
// n_shards above that: the trees' level L (the first with ceil(n / 2^L) <= 4,096 nodes) is
// folded straight from the leaves by a kernel of its own into a scratch buffer
// (rs2k_launch_merkle_trees d_scratch) and the pair-leaf root folds its first L levels into its
// loads (L <= 4); the codec plans take up to 128 blocks of 512 (W <= 65536; jobs above 64 blocks
// run from device memory, CodecJobBig).  That covers every n_shards reed-solomon-simd admits for
// both codes (up to 49,155, the reference's own bound, config.rs:446-460); beyond,
// RS2_E_INCOMPATIBLE_PARAMETERS from the rate check.  Full node arrays (recovery-symbol proofs)
// of wider trees are built one level per launch through HBM; blob batches run their wide trees
// a blob at a time.
constexpr int kMaxShards = 16 * kMerkleMaxLeaves - 1;  // n_shards is a u16
// scratch bytes of the trees' folded level for `trees` trees of n leaves (0 when not needed)
size_t tree_scratch_bytes(int64_t trees, int64_t n) {
  if (n <= kMerkleMaxLeaves) return 0;
  int L = 1;
  while (((n + (int64_t(1) << L) - 1) >> L) > kMerkleMaxLeaves) ++L;
  return size_t(trees) * size_t((n + (int64_t(1) << L) - 1) >> L) * 32;
}

// digests (32 B each, at d_out) of `count` symbols of s bytes back to back at d_symbols
inline hipError_t hash_symbols(const void* d_symbols, int64_t count, int s, void* d_out,
                               hipStream_t st) {
  SymbolMap map{reinterpret_cast<const uint8_t*>(d_symbols), nullptr, nullptr, 0, 0, 0, s};
  return rs2k_launch_leaf_hash(map, 1, count, 1, reinterpret_cast<uint8_t*>(d_out), st);
}

// Root of n leaf digests (32 B each, contiguous) by one level launch per tree level
// (merkle.rs:226-266: odd levels padded with the zero node; one leaf is its own root).
int device_merkle_root(const uint8_t* d_digests, uint64_t n, DevBuf& tmp, uint8_t* d_root,
                       hipStream_t st) {
  if (n == 0) {
    HIP_TRY(hipMemsetAsync(d_root, 0, 32, st));
    return RS2_OK;
  }
  const uint64_t half = (n + 1) / 2;
  HIP_TRY(tmp.ensure(size_t(2 * half * 32)));
  uint8_t* a = tmp.as<uint8_t>();
  uint8_t* b = a + half * 32;
  const uint8_t* src = d_digests;
  uint8_t* dst = a;
  for (uint64_t cnt = n; cnt > 1; cnt = (cnt + 1) / 2) {
    HIP_TRY(rs2k_launch_merkle_level(src, int64_t(cnt), dst, st));
    src = dst;
    dst = dst == a ? b : a;
  }
  HIP_TRY(hipMemcpyAsync(d_root, src, 32, hipMemcpyDeviceToDevice, st));
  return RS2_OK;
}

// Pinned staging ring of the host-buffer ABI.  A transfer is cut into slot-sized pieces: the
// DMA of one piece overlaps the host copies (context worker pool) of the others.  Contiguous
// device ranges of a piece move with one hipMemcpyAsync.  A slot is reused only after the event
// of its last DMA, so consecutive calls need no extra synchronisation.
struct Stager {
  static constexpr int kSlots = 4;
  size_t slot_bytes = size_t(32) << 20;
  PinnedBuf ring;
  Event ev[kSlots];  // each slot's last DMA
  int init() { HIP_TRY(ring.ensure(slot_bytes * kSlots)); return RS2_OK; }
  uint8_t* slot(int k) { return static_cast<uint8_t*>(ring.p) + size_t(k % kSlots) * slot_bytes; }
};

// Pinned staging rings are leased per host-buffer call from a per-device pool (a plan no
// longer owns one): 128 MiB of pinned memory is not re-pinned for every new plan, and the rings
// pinned at once are bounded by the host calls in flight, not by the plans alive.
// RS2_STAGING_RINGS (default 0, at most 16) pins that many rings at the first lease, for a
// fixed pinned budget from the start.
struct StagerPool {
  std::mutex mu;
  bool primed = false;
  std::vector<std::unique_ptr<Stager>> free;
};
StagerPool& stager_pool(int device) {
  // never destroyed: pinned rings outlive the HIP runtime's own teardown at process exit
  static StagerPool* pools = new StagerPool[64];
  return pools[std::min(std::max(device, 0), 63)];
}
struct StagerLease {
  int dev;
  std::unique_ptr<Stager> st;
  explicit StagerLease(int device) : dev(device) {
    StagerPool& pool = stager_pool(dev);
    std::lock_guard<std::mutex> lk(pool.mu);
    if (!pool.primed) {
      pool.primed = true;
      for (int i = 0, k = std::min(16, env_int("RS2_STAGING_RINGS", 0)); i < k; ++i) {
        auto sg = std::make_unique<Stager>();
        if (sg->init() != RS2_OK) break;
        pool.free.push_back(std::move(sg));
      }
    }
    if (!pool.free.empty()) {
      st = std::move(pool.free.back());
      pool.free.pop_back();
    } else {
      st = std::make_unique<Stager>();
    }
  }
  ~StagerLease() {
    StagerPool& pool = stager_pool(dev);
    std::lock_guard<std::mutex> lk(pool.mu);
    if (pool.free.size() < 16) pool.free.push_back(std::move(st));  // else unpinned here
  }
  StagerLease(const StagerLease&) = delete;
  StagerLease& operator=(const StagerLease&) = delete;
};

struct Piece {
  std::vector<Seg> frags;  // h / d of each fragment; the slot holds them back to back
};

std::vector<Piece> cut_pieces(const std::vector<Seg>& segs, size_t slot) {
  std::vector<Piece> out;
  size_t fill = slot;
  for (const auto& g : segs) {
    size_t off = 0;
    while (off < g.len) {
      if (fill == slot) {
        out.emplace_back();
        fill = 0;
      }
      const size_t take = std::min(g.len - off, slot - fill);
      out.back().frags.push_back({g.h + off, g.d + off, take});
      off += take;
      fill += take;
    }
  }
  return out;
}

// one hipMemcpyAsync per run of fragments that are contiguous on the device
hipError_t piece_dma(const Piece& pc, uint8_t* slot, bool to_host, hipStream_t st) {
  size_t o = 0;
  for (size_t i = 0; i < pc.frags.size();) {
    size_t j = i + 1, len = pc.frags[i].len;
    while (j < pc.frags.size() && pc.frags[j].d == pc.frags[j - 1].d + pc.frags[j - 1].len) {
      len += pc.frags[j].len;
      ++j;
    }
    const hipError_t e =
        to_host ? hipMemcpyAsync(slot + o, pc.frags[i].d, len, hipMemcpyDeviceToHost, st)
                : hipMemcpyAsync(pc.frags[i].d, slot + o, len, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    o += len;
    i = j;
  }
  return hipSuccess;
}

std::vector<Seg> slot_view(const Piece& pc, uint8_t* slot) {
  std::vector<Seg> v;
  size_t o = 0;
  for (const auto& f : pc.frags) {
    v.push_back({f.h, slot + o, f.len});
    o += f.len;
  }
  return v;
}

// Caller buffers page-locked with rs2_host_register: start -> length.  A transfer segment whose
// host range lies wholly inside one moves by DMA straight from / to it, without the ring.
std::mutex g_reg_mu;
std::map<uintptr_t, size_t> g_reg;

bool host_registered(const uint8_t* h, size_t len) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(h);
  std::lock_guard<std::mutex> lk(g_reg_mu);
  auto it = g_reg.upper_bound(p);
  if (it == g_reg.begin()) return false;
  --it;
  return p >= it->first && p + len <= it->first + it->second;
}

// Runs of segments contiguous on both sides (a caller's sliver rows laid out back to back, as
// on the device) that lie in registered host memory and reach kDirectMin bytes -> one
// hipMemcpyAsync each on st; the rest returned for the ring (a DMA call per scattered sliver
// costs more than staging it: decode inputs of randomly chosen slivers stay staged).
constexpr size_t kDirectMin = size_t(4) << 20;
std::vector<Seg> issue_direct(const std::vector<Seg>& segs, bool to_host, hipStream_t st,
                              hipError_t* err, bool* any) {
  std::vector<Seg> staged;
  *err = hipSuccess;
  *any = false;
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (g_reg.empty()) return segs;
  }
  std::vector<Seg> runs;
  std::vector<std::pair<size_t, size_t>> span;  // [first, last) segment index of each run
  for (size_t i = 0; i < segs.size(); ++i) {
    const Seg& g = segs[i];
    if (!runs.empty() && g.h == runs.back().h + runs.back().len &&
        g.d == runs.back().d + runs.back().len) {
      runs.back().len += g.len;
      span.back().second = i + 1;
    } else {
      runs.push_back(g);
      span.push_back({i, i + 1});
    }
  }
  for (size_t r = 0; r < runs.size(); ++r) {
    const Seg& g = runs[r];
    if (g.len < kDirectMin || !host_registered(g.h, g.len)) {
      for (size_t i = span[r].first; i < span[r].second; ++i) staged.push_back(segs[i]);
      continue;
    }
    *any = true;
    const hipError_t e = to_host ? hipMemcpyAsync(g.h, g.d, g.len, hipMemcpyDeviceToHost, st)
                                 : hipMemcpyAsync(g.d, g.h, g.len, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) {
      *err = e;
      break;
    }
  }
  return staged;
}

// host -> device, enqueued on st (the host copies are done when this returns; the DMA is not;
// registered caller memory is read by the DMA itself, which every host-buffer call waits for
// before it returns)
int stage_h2d(Context* ctx, Stager& sg, const std::vector<Seg>& segs_all, hipStream_t st) {
  RS2_TRY(sg.init());
  hipError_t de;
  bool any;
  const std::vector<Seg> segs = issue_direct(segs_all, false, st, &de, &any);
  HIP_TRY(de);
  const std::vector<Piece> pcs = cut_pieces(segs, sg.slot_bytes);
  for (size_t k = 0; k < pcs.size(); ++k) {
    const int sl = int(k % Stager::kSlots);
    HIP_TRY(sg.ev[sl].sync());
    par_copy(ctx->pool, slot_view(pcs[k], sg.slot(sl)), false);
    HIP_TRY(piece_dma(pcs[k], sg.slot(sl), false, st));
    HIP_TRY(sg.ev[sl].record(st));
  }
  return RS2_OK;
}

// device -> host after the work queued on st; returns when every byte is in the host buffers
int stage_d2h(Context* ctx, Stager& sg, const std::vector<Seg>& segs_all, hipStream_t st) {
  RS2_TRY(sg.init());
  hipError_t de;
  bool any;
  const std::vector<Seg> segs = issue_direct(segs_all, true, st, &de, &any);
  HIP_TRY(de);
  if (segs.empty()) {
    if (any) HIP_TRY(hipStreamSynchronize(st));
    return RS2_OK;
  }
  const std::vector<Piece> pcs = cut_pieces(segs, sg.slot_bytes);
  auto issue = [&](size_t k) -> int {
    const int sl = int(k % Stager::kSlots);
    HIP_TRY(sg.ev[sl].sync());
    HIP_TRY(piece_dma(pcs[k], sg.slot(sl), true, st));
    HIP_TRY(sg.ev[sl].record(st));
    return RS2_OK;
  };
  for (size_t k = 0; k < pcs.size() && k < size_t(Stager::kSlots); ++k)
    RS2_TRY(issue(k));
  for (size_t k = 0; k < pcs.size(); ++k) {
    const int sl = int(k % Stager::kSlots);
    HIP_TRY(sg.ev[sl].sync());
    par_copy(ctx->pool, slot_view(pcs[k], sg.slot(sl)), true);
    if (k + Stager::kSlots < pcs.size()) RS2_TRY(issue(k + Stager::kSlots));
  }
  return RS2_OK;
}

// Opt-in stage profiler of a plan or a verifier: events recorded between launches on a stream.
struct Prof {
  bool on = false;
  std::vector<hipEvent_t> free_events;
  std::vector<std::pair<std::string, hipEvent_t>> pending;  // "" = start mark
  std::map<std::string, std::pair<double, uint32_t>> acc;   // name -> (total ms, launches)
  std::vector<std::string> order;
  Prof() = default;
  Prof(const Prof&) = delete;
  Prof& operator=(const Prof&) = delete;
  ~Prof() {
    for (auto& e : free_events) (void)hipEventDestroy(e);
    for (auto& pe : pending) (void)hipEventDestroy(pe.second);
  }
};

}  // namespace
}  // namespace rs2

using namespace rs2;

// =============================================================================================
// plans
// =============================================================================================
struct rs2_plan {
  Context* ctx = nullptr;
  hipStream_t stream = nullptr;
  // the systematic-column codec runs beside the row codec on `side` (fork / join events)
  hipStream_t side = nullptr;
  // the same role for split encodes (rs2_encode_device_split_async), at the device's greatest
  // stream priority; created on first use
  hipStream_t side_hi = nullptr;
  Event fork_ev, join_ev, copy_ev;
  // the row codec's padded tail rows (a few workgroups) beside its main launch; created on
  // first use
  hipStream_t aux = nullptr;
  Event aux_ev;
  Event leaf_ev;                       // the side stream's leaf hashes (run A) are done
  Event enc_done;                      // the last encode's work (guards re-binding its arrays)
  uint16_t n = 0, kp = 0, ks = 0, s = 0;
  uint64_t blob_len = 0;
  // encode
  PlannedJob row, col_sys, col_rep;
  JobMem row_mem, col_sys_mem, col_rep_mem;
  DevBuf both, leaves, pairs, blob_id, sys_a_src, sys_a_dst;
  DevBuf int_primary, int_secondary;   // internal sliver buffers (compute_metadata / host API)
  DevBuf dev_blob;                     // host-API staging of the blob / decode output
  const void* bound_primary = nullptr;
  const void* bound_secondary = nullptr;
  bool sys_fused = false;              // systematic secondary slivers written by col_sys
  // the systematic primary slivers (= the blob's zero-padded rows) written by col_sys from its
  // own loads of the blob (InBlock::copy2_base); the padded last rows come from tail_rows
  bool prim_fused = false;
  DevBuf tail_rows;
  DevBuf tree_scratch;                 // n_shards > 4096: the trees' first level
  DevBuf tile_ctr;                     // pipelined codec launch sites' tile counters (kCtr*)
  const void* bound_both = nullptr;
  // blob batches (rs2_encode_batch_*): per-blob repair quadrants and leaf digests, the blob
  // lengths on the device (and the host copy they were uploaded from), the host-buffer form's
  // device blobs / slivers
  DevBuf batch_both, batch_leaves, batch_lens, batch_blob, batch_primary, batch_secondary,
      batch_hashes, batch_ids;
  std::vector<uint64_t> batch_lens_h;
  // decode (two slots so back-to-back async decodes never overwrite live arrays)
  DecodeSlot dec[2];
  int dec_slot = 0;
  // decode batches (rs2_decode_batch_*): the device arrays of one chunk's jobs, two slots taken
  // in turn like `dec`; the host-buffer form's device slivers and blobs
  BatchDecodeSlot dbatch[2];
  int dbatch_slot = 0;
  DevBuf dbatch_in, dbatch_out;
  // host-buffer API: pinned staging ring, a copy stream for the sliver D2H (released by a split
  // encode as soon as the primary slivers are final), row gather offsets of the Default check
  Stager* stage = nullptr;  // the pinned ring leased for the host-buffer call in progress
  hipStream_t io = nullptr;
  rs2_verifier* check_v = nullptr;
  DevBuf check_src, check_rows, check_roots;
  std::vector<int64_t> check_src_h;
  // verified decode batches (rs2_decode_and_verify_batch_*): one window's row and slot tables,
  // gathered rows and roots (Default), re-encoded slivers, hashes and ids (Strict), the call's
  // blob lengths; the host-buffer form's metadata and verdicts.  vb_done: the last call's work,
  // which the next call's stream waits for before it reuses them.
  DevBuf vb_row_tab, vb_slot_tab, vb_rows, vb_roots, vb_primary, vb_secondary, vb_hashes, vb_ids,
      vb_lens, vb_h_hashes, vb_h_ids, vb_h_verdict;
  Event vb_done;
  Prof prof;  // opt-in stage profiler (rs2_profile_*)
  ~rs2_plan() {  // (the Event members go after this body: after every stream, as dec[].done always did)
    if (aux) (void)hipStreamDestroy(aux);
    if (side) (void)hipStreamDestroy(side);
    if (side_hi) (void)hipStreamDestroy(side_hi);
    if (io) (void)hipStreamDestroy(io);
    if (check_v) rs2_verifier_destroy(check_v);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// Batched sliver verification state (no reference counterpart: the storage node verifies
// slivers one by one on a thread pool, walrus-service/src/node.rs:2615-2633).
struct rs2_verifier {
  Context* ctx = nullptr;
  hipStream_t stream = nullptr;
  uint16_t n = 0, k = 0, s = 0;
  PlannedJob job;
  JobMem mem;
  DevBuf input, leaves, roots;
  DevBuf repair;  // the slivers' repair symbols, [count][n - k][s]
  DevBuf tree_scratch;  // n > 4096: the trees' first level
  // recovery symbols with proofs: full trees, targets, outputs of the host-buffer form
  DevBuf nodes, targets, sym_out, proof_out;
  PinnedBuf h_in, h_out;  // host-buffer forms: slivers in, roots / symbols / proofs out
  int axis = 0;
  std::vector<uint16_t> targets_h;  // alive until the upload of the last call has landed
  // sliver recovery (rs2_verifier_recover_slivers_device_async): the chunk slots of the batched
  // decodes and the slots of the per-sliver ones, each pair taken in turn behind `done` events
  // like a plan's; a window's expected roots and skip mask; a window's roots when the caller
  // wants none; the proof check's per-sliver table and leaf digests
  BatchDecodeSlot rbatch[2];
  int rbatch_slot = 0;
  DecodeSlot rdec[2];
  int rdec_slot = 0;
  DevBuf verdict_in, window_roots, per_sliver, sym_digests;
  DevBuf requests;  // bulk recovery symbols: a chunk of the request table (at most kRequestChunk)
  Prof prof;  // opt-in stage profiler of the recovery call (rs2_verifier_profile_*)
  // recorded on the caller's stream after each *_device_async call: destroy waits on it before
  // its buffers go back to the arena as quiesced (they may be handed out again at once)
  Event done;
  ~rs2_verifier() {
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// Mixed sliver verification state (rs2_sliver_checker_*): bound to n_shards only; every sliver of
// a call has its own axis and symbol size (node.rs:2615-2633 verifies what a node receives, from
// many blobs at once).
struct rs2_sliver_checker {
  Context* ctx = nullptr;
  hipStream_t stream = nullptr;
  uint16_t n = 0;
  // per axis: the code's template (planned once, re-planned only when the block limit changed),
  // its job with the transform tables attached, and its mixing tables on the device
  SliverAxisCode codes[2];
  bool bound[2] = {false, false};
  DevBuf mix[2];
  // a window's scratch: gathered slivers, repair symbols, leaves, roots by slot; its tables
  DevBuf gathered, repair, leaves, slot_roots, tables;
  // groups the group launch cannot take run through this verifier, re-pointed per group
  rs2_verifier* single = nullptr;
  // host-buffer form: slivers in, roots and verdicts out
  DevBuf input, out;
  PinnedBuf h_in, h_out;
  // mixed recovery (rs2_sliver_checker_recover_device_async): the chunk slots of the range
  // launches and the slots of the per-sliver decodes, as a verifier's; mixed proof check: the
  // per-sliver tables and the leaf digests
  BatchDecodeSlot rbatch[2];
  int rbatch_slot = 0;
  DecodeSlot rdec[2];
  int rdec_slot = 0;
  DevBuf per_sliver, sym_digests;
  DevBuf nodes;  // mixed recovery symbols: a window's trees, slot after slot
  Event done;  // as rs2_verifier::done
  ~rs2_sliver_checker() {
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// Device 1D codec over many independent codewords ("lines") with strided layouts: the
// building block of the partitioned (multi-GPU) 2D code and of batched recovery symbols.
// The encode job is planned once per layout and re-based per call (the base pointers travel
// in the kernel argument); decodes are planned per erasure pattern in two slots, each
// guarded by an event so an in-flight launch never sees its arrays rewritten.
struct rs2_codec {
  Context* ctx = nullptr;
  uint16_t n = 0, k = 0, s = 0;
  PlannedJob enc;
  JobMem enc_mem;
  int64_t enc_key[4] = {-1, -1, -1, -1};
  Event enc_done;
  DecodeSlot dec[2];
  int dec_slot = 0;
};

namespace {

// Record a stage boundary on `st` (no-op unless profiling).  The stage's time is the span
// from the previous mark on this plan; a mark named "" only starts a span.
void mark(Prof* prof, const char* name, hipStream_t st) {
  auto& pr = *prof;
  if (!pr.on) return;
  hipEvent_t e;
  if (!pr.free_events.empty()) {
    e = pr.free_events.back();
    pr.free_events.pop_back();
  } else if (hipEventCreate(&e) != hipSuccess) {
    return;
  }
  (void)hipEventRecord(e, st);
  pr.pending.emplace_back(name, e);
}

void mark(rs2_plan* p, const char* name, hipStream_t st) { mark(&p->prof, name, st); }

// one more span of `ms` under `name` in the profiler's histogram
void prof_add(Prof& pr, const std::string& name, double ms) {
  auto it = pr.acc.find(name);
  if (it == pr.acc.end()) {
    pr.order.push_back(name);
    it = pr.acc.emplace(name, std::make_pair(0.0, 0u)).first;
  }
  it->second.first += ms;
  it->second.second += 1;
}

// host time since t0 under `name` (profiling on): the erasure-pattern planning of a decode
void prof_host(Prof* prof, const char* name,
               std::chrono::steady_clock::time_point t0) {
  auto& pr = *prof;
  if (!pr.on) return;
  const double ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  host_trace(name, ms);
  prof_add(pr, name, ms);
}

void prof_host(rs2_plan* p, const char* name, std::chrono::steady_clock::time_point t0) {
  prof_host(&p->prof, name, t0);
}

void prof_collect(Prof& pr) {
  hipEvent_t prev = nullptr;
  for (auto& pe : pr.pending) {
    (void)hipEventSynchronize(pe.second);
    if (prev && !pe.first.empty()) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, prev, pe.second) == hipSuccess) prof_add(pr, pe.first, ms);
    }
    prev = pe.second;
  }
  for (auto& pe : pr.pending) pr.free_events.push_back(pe.second);
  pr.pending.clear();
}

// Synchronise on the pending marks, hand out the per-stage totals (names: 32-byte NUL-padded
// slots) and reset them.
int prof_read(Prof& pr, uint32_t max_stages, char* names, double* total_ms, uint32_t* launches,
              uint32_t* n_stages) {
  prof_collect(pr);
  uint32_t k = 0;
  for (const auto& name : pr.order) {
    if (k >= max_stages) break;
    const auto& v = pr.acc[name];
    if (names) {
      std::memset(names + 32 * size_t(k), 0, 32);
      std::strncpy(names + 32 * size_t(k), name.c_str(), 31);
    }
    if (total_ms) total_ms[k] = v.first;
    if (launches) launches[k] = v.second;
    ++k;
  }
  *n_stages = k;
  pr.acc.clear();
  pr.order.clear();
  return RS2_OK;
}

int check_axis(int axis) {
  if (axis == RS2_AXIS_PRIMARY || axis == RS2_AXIS_SECONDARY) return RS2_OK;
  return fail(RS2_E_INVALID_ARGUMENT, "bad axis");
}
int check_value(int check) {
  if (check == RS2_CHECK_SKIP || check == RS2_CHECK_DEFAULT || check == RS2_CHECK_STRICT)
    return RS2_OK;
  return fail(RS2_E_INVALID_ARGUMENT, "bad consistency check");
}

// The count rule of a batch call (`what`: "blobs in a batch", "slivers in a call"): n == 0 sets
// *empty (the call returns RS2_OK); above 65535: refused; then !required is "null argument".
int batch_count(uint32_t n, const char* what, bool required, bool* empty) {
  *empty = n == 0;
  if (n <= 65535) return n == 0 || required ? RS2_OK : fail(RS2_E_INVALID_ARGUMENT, "null argument");
  return fail(RS2_E_INVALID_ARGUMENT, std::string("more than 65535 ") + what);
}
// The outcome of slot i's validation code rc: stored in status_out[i], or returned when status_out
// is null and rc is an error; *accepted says whether the item takes part in the call.
int slot_outcome(int rc, int* status_out, size_t i, bool* accepted) {
  *accepted = rc == RS2_OK;
  if (status_out) status_out[i] = rc;
  return status_out ? RS2_OK : rc;
}
// fn(a, b) for every maximal run [a, b) of [first, last) whose slots (slot_of(i)) are
// neighbours; stops at fn's first error.
template <class SlotOf, class Fn>
int for_each_run(size_t first, size_t last, SlotOf slot_of, Fn fn) {
  for (size_t a = first; a < last;) {
    size_t b = a + 1;
    while (b < last && slot_of(b) == slot_of(b - 1) + 1) ++b;
    RS2_TRY(fn(a, b));
    a = b;
  }
  return RS2_OK;
}
// stats_out[i] = the i-th counter ("null argument" without stats_out)
int read_stats(uint64_t* stats_out, std::initializer_list<const std::atomic<uint64_t>*> counters) {
  if (!stats_out) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  for (const auto* c : counters) *stats_out++ = c->load(std::memory_order_relaxed);
  return RS2_OK;
}

int64_t primary_len(const rs2_plan* p) { return int64_t(p->ks) * p->s; }
int64_t secondary_len(const rs2_plan* p) { return int64_t(p->kp) * p->s; }

// (Re)build the three encode jobs for the given device sliver buffers.  The offset / mixing
// uploads go on `st`, the stream the codecs are launched on next, so they land before the
// kernels read them; the device arrays are shared by every encode of the plan, so an encode
// still in flight on another stream is waited for before they are rewritten.
int bind_encode_buffers(rs2_plan* p, uint8_t* d_primary, uint8_t* d_secondary, hipStream_t st,
                        uint8_t* d_both = nullptr) {
  if (!d_both) d_both = p->both.as<uint8_t>();
  if (p->bound_primary == d_primary && p->bound_secondary == d_secondary &&
      p->bound_both == d_both)
    return RS2_OK;
  HIP_TRY(p->enc_done.sync());
  p->bound_primary = p->bound_secondary = p->bound_both = nullptr;  // valid after a full rebind
  const int64_t s = p->s, n = p->n, kp = p->kp, ks = p->ks;
  // rows: secondary encoding (K = K_s) of primary slivers 0..K_p -> secondary slivers K_s..n
  RS2_TRY(plan_encode(
      uint32_t(ks), uint32_t(n - ks), int(s), d_primary, ks * s, [&](uint32_t c) { return int64_t(c) * s; },
      d_secondary, s, [&](uint32_t j) { return (ks + int64_t(j)) * kp * s; }, INT64_MAX, p->row));
  RS2_TRY(bind_job(p->ctx, p->row, p->row_mem, st));
  // systematic columns c < K_s: primary encoding (K = K_p) -> primary slivers K_p..n, column c
  RS2_TRY(plan_encode(
      uint32_t(kp), uint32_t(n - kp), int(s), d_primary, s, [&](uint32_t r) { return int64_t(r) * ks * s; },
      d_primary, s, [&](uint32_t j) { return (kp + int64_t(j)) * ks * s; }, INT64_MAX, p->col_sys));
  // the column loads are exactly the systematic secondary slivers (secondary c, row r =
  // primary r, column c): write them out from the same loads instead of a transpose pass
  p->sys_fused = false;
  if (s >= 4) {
    set_copy(p->col_sys, d_secondary, kp * s, INT64_MAX, [&](uint32_t r) { return int64_t(r) * s; });
    p->sys_fused = copy_covered(p->col_sys);
  }
  RS2_TRY(bind_job(p->ctx, p->col_sys, p->col_sys_mem, st));
  // the column loads are also every byte of the blob: when one shared-input block holds the
  // K_p rows in order (position r at r * K_s * s), col_sys reads the blob in place and writes
  // the systematic primary slivers itself instead of a separate blob copy
  p->prim_fused = false;
  // RS2_FUSE_BLOB=0: the separate blob copy (A/B knob)
  static const bool fuse_env = env_int("RS2_FUSE_BLOB", 1) != 0;
  if (fuse_env && p->sys_fused && p->col_sys.mode == kModeCols && p->col_sys.job.n_in == 1 &&
      p->col_sys.job.in[0].count == int(kp)) {
    bool in_order = true;
    for (int64_t r = 0; r < kp; ++r) in_order &= p->col_sys.offs[size_t(r)] == r * ks * s;
    const int64_t r_full = std::min<int64_t>(kp, int64_t(p->blob_len) / (ks * s));
    if (in_order && r_full < kp) HIP_TRY(p->tail_rows.ensure(size_t((kp - r_full) * ks * s)));
    p->prim_fused = in_order;
  }
  // repair columns c >= K_s: from secondary slivers K_s..n -> the both-repair quadrant
  RS2_TRY(plan_encode(
      uint32_t(kp), uint32_t(n - kp), int(s), d_secondary + ks * kp * s, kp * s,
      [&](uint32_t r) { return int64_t(r) * s; }, d_both, s,
      [&](uint32_t j) { return int64_t(j) * (n - ks) * s; }, INT64_MAX, p->col_rep));
  RS2_TRY(bind_job(p->ctx, p->col_rep, p->col_rep_mem, st));
  p->bound_primary = d_primary;
  p->bound_secondary = d_secondary;
  p->bound_both = d_both;
  return RS2_OK;
}

// messages at least this large (K_p * K_s * s bytes) get the extra stream overlap in
// encode_device (tail rows beside the main row launch, leaf hashes split across streams)
constexpr int64_t kBigMessage = int64_t(64) << 20;

int encode_device(rs2_plan* p, const uint8_t* d_blob, uint8_t* d_primary, uint8_t* d_secondary,
                  uint8_t* d_hashes, uint8_t* d_blob_id, hipStream_t st, bool need_slivers,
                  hipStream_t prim_st = nullptr) {
  const int64_t s = p->s, n = p->n, kp = p->kp, ks = p->ks;
  const int64_t msg = kp * ks * s;
  RS2_TRY(bind_encode_buffers(p, d_primary, d_secondary, st));
  // The plan's buffers (repair quadrant, leaves, tile counters) serve one encode at a time: an
  // encode queued on another stream than the previous one's runs after it on the device.
  HIP_TRY(p->enc_done.wait_on(st));
  // A split encode's primary slivers (blob copy + systematic-column codec on the side stream)
  // are the critical path of the caller's next step (a decode, a send).  Round 1 ran them on a
  // high-priority side stream; with the bench's steps correctly ordered (round 2: each encode
  // waits for the last reader of its buffers) that costs 3.73 -> 4.10 ms per step, so the side
  // stream keeps the default priority unless RS2_SIDE_PRIORITY=1 (A/B knob).
  hipStream_t side = p->side;
  static const bool side_priority = env_int("RS2_SIDE_PRIORITY", 0) != 0;
  if (prim_st && side_priority) {
    if (!p->side_hi) {
      int lo_pri = 0, hi_pri = 0;
      HIP_TRY(hipDeviceGetStreamPriorityRange(&lo_pri, &hi_pri));
      HIP_TRY(hipStreamCreateWithPriority(&p->side_hi, hipStreamNonBlocking, hi_pri));
    }
    side = p->side_hi;
  }
  // tile counters of the pipelined codec launches below, one set per launch site (they may run
  // at once on different streams); zeroed once, and re-zeroed by each launch's last workgroup
  if (!p->tile_ctr.p) {
    HIP_TRY(p->tile_ctr.ensure(4 * kTileCtrWords * 4));
    HIP_TRY(hipMemsetAsync(p->tile_ctr.p, 0, 4 * kTileCtrWords * 4, st));
  }
  uint32_t* const ctr = p->tile_ctr.as<uint32_t>();
  mark(p, "", st);
  // Two streams.  Side: the systematic-column codec, which reads the blob's rows in place and
  // (fused, prim_fused) writes the systematic primary slivers (= the zero-padded blob rows) from
  // the same loads; else a D2D copy makes those slivers first.  Caller's stream: the row codec
  // -- rows that lie wholly inside the blob straight from d_blob, the padded tail rows from the
  // tail buffer (or, unfused, from the copied slivers) -- then the repair-column codec.  The
  // codec grids fill each other's last, partly empty rounds of workgroups; stage times overlap
  // and each is its own span.
  // The blob's partial last row (and any rows past its end), zero-padded, in a small buffer that
  // both codecs read in place of the missing rows (fused path).
  const int64_t r_full = std::min<int64_t>(kp, int64_t(p->blob_len) / (ks * s));
  // BlobEncoder::compute_metadata (blob_encoding.rs:406-486) keeps no sliver: with the blob read
  // in place (fused) the systematic slivers are never materialised, only hashed
  const bool meta_only = !need_slivers && p->prim_fused && p->sys_fused;
  const uint8_t* tail_base = nullptr;
  if (p->prim_fused && r_full < kp) {
    const int64_t have = int64_t(p->blob_len) - r_full * ks * s;
    HIP_TRY(p->tail_rows.ensure(size_t((kp - r_full) * ks * s)));  // the plan may have been rebound
    uint8_t* tail = p->tail_rows.as<uint8_t>();
    HIP_TRY(rs2k_launch_tail_rows(d_blob + r_full * ks * s, have, tail, (kp - r_full) * ks * s, st));
    mark(p, "enc_tail_rows", st);
    tail_base = tail - r_full * ks * s;  // row r >= r_full at tail_base + r * K_s * s
  }
  HIP_TRY(p->fork_ev.record(st));
  HIP_TRY(p->fork_ev.wait_on(side));
  mark(p, "", side);
  if (p->prim_fused) {
    CodecJobBig cj = p->col_sys.job;
    cj.in[0].base = d_blob;
    cj.in[0].copy2_base = d_primary;
    if (r_full < kp) {
      cj.in[0].alt_base = tail_base;
      cj.in[0].alt_from = int(r_full);
    }
    if (meta_only) {
      // compute_metadata: no systematic sliver is written (neither the secondary copy-out nor
      // the primary one); their leaves are hashed from the blob and the tail buffer below
      cj.in[0].copy_off = nullptr;
      cj.in[0].copy2_base = nullptr;
    }
    HIP_TRY(launch_codec_c(p->col_sys.C, cj, int(ks), p->col_sys.n_z, p->col_sys.mode, side, 1, 0,
                           0, 0, ctr));
  } else {
    if (p->blob_len)
      HIP_TRY(hipMemcpyAsync(d_primary, d_blob, p->blob_len, hipMemcpyDeviceToDevice, side));
    if (uint64_t(msg) > p->blob_len)
      HIP_TRY(hipMemsetAsync(d_primary + p->blob_len, 0, msg - p->blob_len, side));
    mark(p, "enc_blob_copy", side);
    HIP_TRY(p->copy_ev.record(side));
    HIP_TRY(launch_job(p->col_sys, int(ks), side, ctr));
  }
  mark(p, "enc_cols_sys_codec", side);
  HIP_TRY(p->join_ev.record(side));
  // all primary slivers are final here (systematic rows + the column code's repair rows):
  // work the caller queues on prim_st next (a decode, a D2H to the NIC) starts now, beside
  // the secondary codecs and the hashing still running on st
  if (prim_st) HIP_TRY(p->join_ev.wait_on(prim_st));
  // RS2_TAIL_AUX=1 (A/B): the padded tail rows (a few workgroups) on a stream of their own
  // beside the main row launch instead of after it, the repair-column codec waiting for both.
  // Off by default since round 5: beside the persistent row kernel the tail's workgroups wait
  // for CUs anyway (the kernel trace shows them finishing with it), and the step is 88.1-88.3
  // vs 87.7-87.9 GiB/s without them on their own stream (five interleaved pairs,
  // profiles/r05/exp/tailaux/)
  static const bool tail_aux = env_int("RS2_TAIL_AUX", 0) == 1;
  // (large blobs only: for small ones the extra stream and launch cost more than the tail, and
  // many plans encoding at once share the device's few hardware queues: C3's 16 plans on 16
  // streams measured 12.1 vs 13.6 GiB/s with it)
  const bool big = msg >= kBigMessage;
  const bool aux_tail = p->prim_fused && r_full < kp && r_full > 0 && tail_aux && big;
  if (aux_tail) {
    if (!p->aux) HIP_TRY(hipStreamCreateWithFlags(&p->aux, hipStreamNonBlocking));
    HIP_TRY(p->fork_ev.wait_on(p->aux));
    mark(p, "", p->aux);
    CodecJobBig tail = p->row.job;
    tail.line_base = int(r_full);
    for (int b = 0; b < tail.n_in; ++b) tail.in[b].base = tail_base;
    HIP_TRY(launch_codec_c(p->row.C, tail, int(kp - r_full), p->row.n_z, p->row.mode, p->aux, 1,
                           0, 0, 0, ctr + 2 * kTileCtrWords));
    mark(p, "enc_rows_tail", p->aux);
    HIP_TRY(p->aux_ev.record(p->aux));
  }
  mark(p, "", st);
  if (r_full > 0) {
    CodecJobBig from_blob = p->row.job;  // same layout: blob row r is primary sliver r
    for (int b = 0; b < from_blob.n_in; ++b) from_blob.in[b].base = d_blob;
    HIP_TRY(launch_codec_c(p->row.C, from_blob, int(r_full), p->row.n_z, p->row.mode, st, 1, 0, 0,
                           0, ctr + kTileCtrWords));
  }
  if (aux_tail) {
    HIP_TRY(p->aux_ev.wait_on(st));
  } else if (r_full < kp) {
    CodecJobBig tail = p->row.job;
    tail.line_base = int(r_full);
    if (p->prim_fused)  // the padded rows from the tail buffer (filled above, on st)
      for (int b = 0; b < tail.n_in; ++b) tail.in[b].base = tail_base;
    else  // from the systematic primary slivers once the side stream's copy has landed
      HIP_TRY(p->copy_ev.wait_on(st));
    HIP_TRY(launch_codec_c(p->row.C, tail, int(kp - r_full), p->row.n_z, p->row.mode, st, 1, 0, 0,
                           0, ctr + 2 * kTileCtrWords));
  }
  mark(p, "enc_rows_codec", st);
  HIP_TRY(launch_job(p->col_rep, int(n - ks), st, ctr + 3 * kTileCtrWords));
  mark(p, "enc_cols_rep_codec", st);
  // leaf hashes of all n x n symbols, 2n Merkle trees, root and blob id.  The primary slivers'
  // leaves (run A) are hashed on the side stream as soon as the systematic-column codec is done,
  // beside the row / repair-column codecs; the secondary-side runs B and C here after them.
  SymbolMap map{d_primary, d_secondary, p->both.as<uint8_t>(), int(n), int(kp), int(ks), int(s)};
  // RS2_SPLIT_LEAF=0: one leaf launch after the join (A/B)
  static const bool split_leaf = env_int("RS2_SPLIT_LEAF", 1) != 0;
  const bool split = split_leaf && p->sys_fused && big;  // (C3 streams: 11.1 vs 13.6 GiB/s)
  if (meta_only) {
    // run A (rows of K_s symbols, leaf (r, c) at r*n + c) from where the rows are: the blob's
    // whole rows in place, its zero-padded tail rows in the tail buffer, the repair rows K_p..n
    // in the primary scratch; then runs B and C (the secondary side) as below
    hipStream_t sa = split ? side : st;
    if (!split) HIP_TRY(p->join_ev.wait_on(st));
    mark(p, "", sa);
    auto rows_run = [&](const uint8_t* base, int64_t r0, int64_t rows) -> int {
      if (rows <= 0) return RS2_OK;
      SymbolMap rm{base, nullptr, nullptr, int(n), int(rows), int(ks), int(s)};
      HIP_TRY(rs2k_launch_leaf_hash(rm, 4, rows * n, 1, p->leaves.as<uint8_t>() + r0 * n * 32, sa));
      return RS2_OK;
    };
    int rc2 = rows_run(d_blob, 0, r_full);
    if (rc2 == RS2_OK && r_full < kp) rc2 = rows_run(tail_base + r_full * ks * s, r_full, kp - r_full);
    if (rc2 == RS2_OK) rc2 = rows_run(d_primary + kp * ks * s, kp, n - kp);
    if (rc2 != RS2_OK) return rc2;
    mark(p, "enc_leaf_hash_a", sa);
    if (split) HIP_TRY(p->leaf_ev.record(side));
    mark(p, "", st);
    HIP_TRY(rs2k_launch_leaf_hash(map, 3, n * n, 1, p->leaves.as<uint8_t>(), st));
    mark(p, "enc_leaf_hash", st);
    if (split) HIP_TRY(p->leaf_ev.wait_on(st));
  } else if (split) {
    mark(p, "", side);
    HIP_TRY(rs2k_launch_leaf_hash(map, 2, n * n, 1, p->leaves.as<uint8_t>(), side));
    mark(p, "enc_leaf_hash_a", side);
    HIP_TRY(p->leaf_ev.record(side));
    mark(p, "", st);
    HIP_TRY(rs2k_launch_leaf_hash(map, 3, n * n, 1, p->leaves.as<uint8_t>(), st));
    mark(p, "enc_leaf_hash", st);
    HIP_TRY(p->leaf_ev.wait_on(st));  // after join_ev on the side stream
  } else {
    HIP_TRY(p->join_ev.wait_on(st));
    mark(p, "", st);
    if (!p->sys_fused) {
      // systematic secondary slivers: secondary c, row r = primary r, column c (c < K_s)
      HIP_TRY(rs2k_launch_symbol_copy(d_primary, p->sys_a_src.as<int64_t>(), ks * s, d_secondary,
                                      p->sys_a_dst.as<int64_t>(), s, int(ks), int(kp), int(s),
                                      INT64_MAX, st));
      mark(p, "enc_sys_transpose", st);
    }
    HIP_TRY(rs2k_launch_leaf_hash(map, 0, n * n, 1, p->leaves.as<uint8_t>(), st));
    mark(p, "enc_leaf_hash", st);
  }
  mark(p, "", st);
  uint8_t* pairs = d_hashes ? d_hashes : p->pairs.as<uint8_t>();
  uint8_t* scratch = nullptr;
  if (const size_t sb = tree_scratch_bytes(2 * n, n)) {
    HIP_TRY(p->tree_scratch.ensure(sb));
    scratch = p->tree_scratch.as<uint8_t>();
  }
  HIP_TRY(rs2k_launch_merkle_trees(p->leaves.as<uint8_t>(), int(n), int(n), int(n), n * 32, 32,
                                   32, n * 32, pairs, 64, st, nullptr, 0, 1, 0, 0, scratch));
  mark(p, "enc_merkle_trees", st);
  HIP_TRY(rs2k_launch_merkle_root(pairs, int(n), p->blob_len,
                                  d_blob_id ? d_blob_id : p->blob_id.as<uint8_t>(), st));
  mark(p, "enc_merkle_root", st);
  HIP_TRY(p->enc_done.record(st));  // st has joined the side stream above
  return RS2_OK;
}

// The metadata alone (BlobEncoder::compute_metadata): the slivers go to the plan's own buffers.
int encode_metadata(rs2_plan* p, const uint8_t* d_blob, uint8_t* d_hashes, uint8_t* d_blob_id,
                    hipStream_t st) {
  HIP_TRY(p->int_primary.ensure(size_t(p->n) * primary_len(p)));
  HIP_TRY(p->int_secondary.ensure(size_t(p->n) * secondary_len(p)));
  return encode_device(p, d_blob, p->int_primary.as<uint8_t>(), p->int_secondary.as<uint8_t>(),
                       d_hashes, d_blob_id, st, false);
}

// Blob batch (the upload relay's many-blob encode, walrus-upload-relay/src/controller.rs:177;
// the client's encode_blobs_as, node_client.rs:3156-3221): n_blobs blobs of this plan's symbol
// size, blob b at d_blobs + b*blob_stride (lens[b] bytes, or the plan's blob_len for all), its
// slivers at d_primary + b*p_stride / d_secondary + b*s_stride (the single-blob layouts), its
// pair hashes at d_hashes + b*64n and BlobId at d_blob_ids + b*32.  Every stage is ONE launch
// over all blobs (the codec grids hold every blob's tiles, the hash grids a blob per grid.y),
// so many small blobs cost no more launches than one large one.
int encode_batch_device(rs2_plan* p, uint32_t n_blobs, const uint8_t* d_blobs, int64_t blob_stride,
                        const uint64_t* lens, uint8_t* d_primary, int64_t p_stride,
                        uint8_t* d_secondary, int64_t s_stride, uint8_t* d_hashes,
                        uint8_t* d_blob_ids, hipStream_t st,
                        const uint64_t* d_lens_ready = nullptr) {
  const int64_t s = p->s, n = p->n, kp = p->kp, ks = p->ks;
  const int64_t msg = kp * ks * s, pl = ks * s, sl = kp * s;
  bool empty;
  RS2_TRY(batch_count(n_blobs, "blobs in a batch",
                      d_primary && d_secondary && d_hashes && d_blob_ids, &empty));
  if (empty) return RS2_OK;
  if (p_stride < n * pl || s_stride < n * sl)
    return fail(RS2_E_INVALID_ARGUMENT, "sliver stride smaller than a blob's slivers");
  std::vector<uint64_t> lv(n_blobs, p->blob_len);
  uint64_t max_len = 0;
  for (uint32_t b = 0; b < n_blobs; ++b) {
    if (lens) lv[b] = lens[b];
    uint16_t sb = 0;
    RS2_TRY(rs2_symbol_size_for_blob(p->n, lv[b], &sb));
    if (sb != p->s) return fail(RS2_E_INVALID_ARGUMENT, "blob length outside the plan's symbol size");
    max_len = std::max(max_len, lv[b]);
  }
  if (max_len && !d_blobs) return fail(RS2_E_INVALID_ARGUMENT, "null blobs");
  if (n_blobs > 1 && int64_t(max_len) > blob_stride)
    return fail(RS2_E_INVALID_ARGUMENT, "blob stride smaller than a blob");
  const int64_t both_b = (n - kp) * (n - ks) * s, leaves_b = n * n * 32;
  HIP_TRY(p->batch_both.ensure(size_t(n_blobs) * both_b));
  HIP_TRY(p->batch_leaves.ensure(size_t(n_blobs) * leaves_b));
  RS2_TRY(bind_encode_buffers(p, d_primary, d_secondary, st, p->batch_both.as<uint8_t>()));
  // d_lens_ready: the caller has the same lengths on the device already (a verified decode
  // batch uploads its call's lengths once, so no run of a window waits for the one before)
  if (!d_lens_ready && lv != p->batch_lens_h) {  // upload the lengths (the host copy stays alive until it lands)
    HIP_TRY(p->enc_done.sync());
    p->batch_lens_h = lv;
    HIP_TRY(p->batch_lens.ensure(lv.size() * 8));
    HIP_TRY(p->ctx->upload(p->batch_lens.p, p->batch_lens_h.data(), lv.size() * 8, st));
  }
  const uint64_t* d_lens = d_lens_ready ? d_lens_ready : p->batch_lens.as<uint64_t>();
  const int B = int(n_blobs);
  mark(p, "", st);
  HIP_TRY(rs2k_launch_batch_blob_copy(d_blobs, blob_stride, d_lens, msg, d_primary, p_stride, B, st));
  mark(p, "enc_blob_copy", st);
  HIP_TRY(launch_codec_c(p->col_sys.C, p->col_sys.job, int(ks), p->col_sys.n_z, p->col_sys.mode,
                         st, B, p_stride, p_stride, s_stride));
  mark(p, "enc_cols_sys_codec", st);
  HIP_TRY(launch_codec_c(p->row.C, p->row.job, int(kp), p->row.n_z, p->row.mode, st, B, p_stride,
                         s_stride, 0));
  mark(p, "enc_rows_codec", st);
  HIP_TRY(launch_codec_c(p->col_rep.C, p->col_rep.job, int(n - ks), p->col_rep.n_z,
                         p->col_rep.mode, st, B, s_stride, both_b, 0));
  mark(p, "enc_cols_rep_codec", st);
  if (!p->sys_fused)
    for (int b = 0; b < B; ++b)
      HIP_TRY(rs2k_launch_symbol_copy(d_primary + b * p_stride, p->sys_a_src.as<int64_t>(), ks * s,
                                      d_secondary + b * s_stride, p->sys_a_dst.as<int64_t>(), s,
                                      int(ks), int(kp), int(s), INT64_MAX, st));
  SymbolMap map{d_primary, d_secondary, p->batch_both.as<uint8_t>(), int(n), int(kp), int(ks),
                int(s), p_stride, s_stride, both_b, leaves_b};
  HIP_TRY(rs2k_launch_leaf_hash(map, 0, n * n, B, p->batch_leaves.as<uint8_t>(), st));
  mark(p, "enc_leaf_hash", st);
  if (const size_t sb = tree_scratch_bytes(2 * n, n)) {
    // trees wider than one wave's slab: a blob at a time through the plan's fold scratch
    // (launches on one stream, so the scratch is reused in order)
    HIP_TRY(p->tree_scratch.ensure(sb));
    for (int b = 0; b < B; ++b)
      HIP_TRY(rs2k_launch_merkle_trees(p->batch_leaves.as<uint8_t>() + b * leaves_b, int(n),
                                       int(n), int(n), n * 32, 32, 32, n * 32, d_hashes + b * n * 64,
                                       64, st, nullptr, 0, 1, 0, 0, p->tree_scratch.as<uint8_t>()));
  } else {
    HIP_TRY(rs2k_launch_merkle_trees(p->batch_leaves.as<uint8_t>(), int(n), int(n), int(n), n * 32,
                                     32, 32, n * 32, d_hashes, 64, st, nullptr, 0, B, leaves_b,
                                     n * 64));
  }
  mark(p, "enc_merkle_trees", st);
  HIP_TRY(rs2k_launch_merkle_root(d_hashes, int(n), p->blob_len, d_blob_ids, st, B, d_lens));
  mark(p, "enc_merkle_root", st);
  HIP_TRY(p->enc_done.record(st));
  return RS2_OK;
}

// Select the slivers a BlobDecoder would use (blob_encoding.rs:904-951): walk the input in
// order, stop once `need` slivers are taken (the item that finds the workspace full has been
// pulled from the iterator: it still counts for the Default check, config.rs:621-640), skip a
// repeated index, drop a sliver of the wrong length or symbol size (lens / sym_sizes may be
// null).  An index >= n_shards is taken like any other -- the reference's BTreeSet accepts any
// u16 -- and makes the column decodes fail with NotEnoughShards later (basic_encoding.rs:
// 400-410: reed-solomon-simd rejects the shard, the error is ignored, decode() then has too
// few).  *pulled = number of input slivers consumed.
int select_slivers(const rs2_plan* p, int axis, uint32_t count, const uint16_t* idx,
                   const uint64_t* lens, const uint16_t* sym_sizes,
                   std::vector<std::pair<uint16_t, uint32_t>>& chosen, uint32_t* pulled = nullptr) {
  const uint32_t need = axis == RS2_AXIS_PRIMARY ? p->kp : p->ks;
  const uint64_t want_len = uint64_t(axis == RS2_AXIS_PRIMARY ? primary_len(p) : secondary_len(p));
  std::vector<uint8_t> seen(65536, 0);
  chosen.clear();
  uint32_t i = 0;
  for (; i < count; ++i) {
    if (chosen.size() == need) {
      ++i;  // pulled, then dropped as surplus
      break;
    }
    const uint16_t q = idx[i];
    if (seen[q]) continue;
    if (lens && lens[i] != want_len) continue;
    if (sym_sizes && sym_sizes[i] != p->s) continue;
    seen[q] = 1;
    chosen.emplace_back(q, i);
  }
  if (pulled) *pulled = std::min(i, count);
  if (chosen.size() != need) return fail(RS2_E_DECODING_UNSUCCESSFUL, "not enough slivers");
  for (const auto& c : chosen)
    if (c.first >= p->n) return fail(RS2_E_NOT_ENOUGH_SHARDS, "not enough shards (sliver index out of range)");
  return RS2_OK;
}

// The decode sequence of a blob plan and of a 1D codec: wait for the slot, list the present
// originals, plan the erasure pattern (unless the slot was planned for the same key), copy the
// present originals that the kernel does not write itself, bind, launch, record the event.
// The copy runs over the decode's own geometry: `lines` lines sp.src_ls / sp.dst_ls apart,
// bytes at or past sp.dst_limit not written.  The copy list is built from sp.present in index
// order (a plan's used to follow the caller's sliver order; the copies are independent, so the
// bytes written are the same).  A source offset of 2^63 or more is negative in sp.present and
// so counts as absent here, as it always did for the decode plan itself.
int run_decode(Context* ctx, DecodeSlot (&slots)[2], int& cursor, DecodeSpec& sp,
               std::vector<int64_t> key, bool may_fuse, int lines, Prof* prof,
               hipStream_t st) {
  DecodeSlot& sl = slots[cursor];
  cursor ^= 1;
  const auto wait_t0 = std::chrono::steady_clock::now();
  HIP_TRY(sl.done.sync());
  if (prof) prof_host(prof, "dec_host_slotwait", wait_t0);
  std::vector<int64_t>& copy_src = sl.copy_src_h;
  std::vector<int64_t>& copy_dst = sl.copy_dst_h;
  copy_src.clear();
  copy_dst.clear();
  for (uint32_t i = 0; i < sp.K; ++i)
    if (sp.present[i] >= 0) {
      copy_src.push_back(sp.present[i]);
      copy_dst.push_back(sp.dst[i]);
    }
  if (prof) mark(prof, "", st);
  const bool run_codec = copy_src.size() < sp.K;
  PlannedJob& pj = sl.job;
  const bool cached = !key.empty() && key == sl.key;
  sl.key.clear();  // valid again only once this call has re-planned successfully
  bool fused = cached && sl.fused;
  const auto host_t0 = std::chrono::steady_clock::now();
  if (run_codec && !cached) {
    // present originals are written by the decode kernel from its own loads when it can
    sp.copy_present = !copy_src.empty() && sp.symbol_size >= 4 && may_fuse;
    RS2_TRY(plan_decode(sp, pj));
    fused = sp.copy_present && copy_covered(pj);
    if (prof) prof_host(prof, "dec_host_plan", host_t0);
  }
  // present originals: straight copies into the output (when not fused into the decode)
  if (!copy_src.empty() && !fused) {
    if (!cached) {
      HIP_TRY(sl.copy_src.ensure(copy_src.size() * 8));
      HIP_TRY(sl.copy_dst.ensure(copy_dst.size() * 8));
      HIP_TRY(ctx->upload(sl.copy_src.p, copy_src.data(), copy_src.size() * 8, st));
      HIP_TRY(ctx->upload(sl.copy_dst.p, copy_dst.data(), copy_dst.size() * 8, st));
    }
    HIP_TRY(rs2k_launch_symbol_copy(sp.src_base, sl.copy_src.as<int64_t>(), sp.src_ls, sp.dst_base,
                                    sl.copy_dst.as<int64_t>(), sp.dst_ls, int(copy_src.size()),
                                    lines, sp.symbol_size, sp.dst_limit, st));
    if (prof) mark(prof, "dec_copy_present", st);
  }
  if (run_codec) {
    if (!cached) {
      const auto bind_t0 = std::chrono::steady_clock::now();
      // (on st, behind its wait for the slivers: the same setup on a stream of its own, so the
      // decode starts the moment the primary slivers are final, measured 81.8 vs 87.4 GiB/s --
      // a decode that takes the CUs earlier delays the encode's chain)
      RS2_TRY(bind_decode(ctx, pj, sl.mem, st));
      if (prof) prof_host(prof, "dec_host_bind", bind_t0);
      if (prof) prof_host(prof, "dec_plan_host", host_t0);
    }
    if (prof) mark(prof, "dec_setup", st);
    HIP_TRY(launch_job(pj, lines, st));
    if (prof) mark(prof, "dec_codec", st);
  }
  HIP_TRY(sl.done.record(st));
  sl.key = std::move(key);
  sl.fused = fused;
  return RS2_OK;
}

// The decode of a blob of `blob_len` bytes from chosen device slivers (sliver i at base + off[i])
// into d_out, and the key that names the job in a decode slot.
void blob_decode_spec(const rs2_plan* p, int axis,
                      const std::vector<std::pair<uint16_t, uint32_t>>& chosen, const uint8_t* base,
                      const uint64_t* off, uint8_t* d_out, uint64_t blob_len, DecodeSpec& sp,
                      std::vector<int64_t>& key) {
  const int64_t s = p->s, n = p->n, kp = p->kp, ks = p->ks;
  const bool prim = axis == RS2_AXIS_PRIMARY;
  const uint32_t K = prim ? uint32_t(kp) : uint32_t(ks);
  sp.K = K;
  sp.R = uint32_t(n) - K;
  sp.symbol_size = int(s);
  sp.present.assign(n, -1);
  sp.src_base = base;
  sp.src_ls = s;  // line = column c (primary) / row r (secondary): symbol c of the sliver
  sp.dst_base = d_out;
  sp.dst_limit = int64_t(blob_len);
  sp.dst.resize(K);
  for (uint32_t i = 0; i < K; ++i) sp.dst[i] = prim ? int64_t(i) * ks * s : int64_t(i) * s;
  sp.dst_ls = prim ? s : ks * s;
  for (auto& c : chosen) sp.present[c.first] = int64_t(off[c.second]);
  key.clear();
  key.reserve(size_t(n) + 5);
  key.push_back(axis);
  key.push_back(int64_t(block_max()));
  key.push_back(int64_t(blob_len));  // sp.dst_limit: rebind keeps the plan, not the limit
  key.push_back(int64_t(reinterpret_cast<uintptr_t>(base)));
  key.push_back(int64_t(reinterpret_cast<uintptr_t>(d_out)));
  key.insert(key.end(), sp.present.begin(), sp.present.end());
}

bool decode_may_fuse() {
  static const bool no_fuse = env_int("RS2_DEC_NOFUSE", 0) != 0;  // A/B knob: RS2_DEC_NOFUSE=1
  return !no_fuse;
}

// Decode from chosen device slivers: sliver i at base + off[i].
int decode_device(rs2_plan* p, int axis, const std::vector<std::pair<uint16_t, uint32_t>>& chosen,
                  const uint8_t* base, const uint64_t* off, uint8_t* d_out, hipStream_t st,
                  uint64_t blob_len) {
  DecodeSpec sp;
  std::vector<int64_t> key;
  blob_decode_spec(p, axis, chosen, base, off, d_out, blob_len, sp, key);
  const int lines = axis == RS2_AXIS_PRIMARY ? int(p->ks) : int(p->kp);
  return run_decode(p->ctx, p->dec, p->dec_slot, sp, std::move(key), decode_may_fuse(), lines,
                    &p->prof,
                    st);
}

// Stream argument of the plan / verifier ABI: NULL = the object's own stream,
// RS2_STREAM_LEGACY ((void*)1) = the HIP null stream (torch's default stream), else a
// hipStream_t.
hipStream_t abi_stream(void* stream, hipStream_t own) {
  if (!stream) return own;
  if (stream == RS2_STREAM_LEGACY) return nullptr;
  return reinterpret_cast<hipStream_t>(stream);
}

hipStream_t pick_stream(rs2_plan* p, void* stream) {
  return abi_stream(stream, p->stream);
}

// Alignment contract of the device entry points (include/walrus_rs2.h): symbol-carrying
// buffers, their offsets and strides are 2-byte aligned (the kernels move symbols with 2-byte
// and possibly misaligned wider accesses, never single bytes of a full element), digest /
// proof / node buffers 16-byte aligned (uint4 accesses).  Checked on the host before anything
// is enqueued; NULL passes (optional outputs; required ones are refused as null arguments).
bool aligned_to(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }
int check_symbol_ptr(const void* p, const char* what) {
  if (aligned_to(p, 2)) return RS2_OK;
  return fail(RS2_E_INVALID_ARGUMENT, std::string(what) + " must be 2-byte aligned");
}
int check_symbol_step(uint64_t v, const char* what) {
  if (v % 2 == 0) return RS2_OK;
  return fail(RS2_E_INVALID_ARGUMENT, std::string(what) + " must be a multiple of 2 bytes");
}
// Strides and offsets of the strided 1D codec: 2-byte aligned like every symbol step and below
// 2^47 (include/walrus_rs2.h), so that the int64 offsets planned from them cannot overflow.
int check_codec_step(uint64_t v, const char* what) {
  RS2_TRY(check_symbol_step(v, what));
  if (v < (uint64_t(1) << 47)) return RS2_OK;
  return fail(RS2_E_INVALID_ARGUMENT, std::string(what) + " must be below 2^47 bytes");
}
int check_digest_ptr(const void* p, const char* what) {
  if (aligned_to(p, 16)) return RS2_OK;
  return fail(RS2_E_INVALID_ARGUMENT, std::string(what) + " must be 16-byte aligned");
}
int check_encode_ptrs(const void* d_blob, const void* d_primary, const void* d_secondary,
                      const void* d_hashes, const void* d_blob_id) {
  RS2_TRY(check_symbol_ptr(d_blob, "d_blob"));
  RS2_TRY(check_symbol_ptr(d_primary, "d_primary"));
  RS2_TRY(check_symbol_ptr(d_secondary, "d_secondary"));
  RS2_TRY(check_digest_ptr(d_hashes, "d_hashes"));
  return check_digest_ptr(d_blob_id, "d_blob_id");
}
int check_decode_ptrs(uint32_t count, const void* d_slivers_base, const uint64_t* sliver_off,
                      const void* d_blob_out) {
  RS2_TRY(check_symbol_ptr(d_slivers_base, "d_slivers_base"));
  for (uint32_t i = 0; i < count; ++i) RS2_TRY(check_symbol_step(sliver_off[i], "sliver_off[i]"));
  return check_symbol_ptr(d_blob_out, "d_blob_out");
}

// ---------------------------------------------------------------------------------------------
// decode batches: many blobs of the plan's symbol size, an erasure pattern per blob
// ---------------------------------------------------------------------------------------------
// One validated blob of a batch call: its slivers (select_slivers: index, position in `off`),
// their offsets from the call's sliver base, its length and its output.
struct BatchItem {
  uint32_t blob = 0;
  uint64_t len = 0;
  std::vector<std::pair<uint16_t, uint32_t>> chosen;
  const uint64_t* off = nullptr;
  uint8_t* out = nullptr;
  // the input indices the decoder consumed (select_slivers' *pulled): what the Default check of
  // a verified batch counts as already verified
  const uint16_t* idx = nullptr;
  uint32_t pulled = 0;
};

// A blob planned for the batch kernel (on a pool thread): its job, narrowed and with the
// arrays it will point into still on the host.
struct BatchBlob {
  bool eligible = false;
  CodecJobBatch job{};
  int C = 1, ppw = kPpwTarget;
  size_t n_off = 0;                  // position offsets in `offs`; the copy offsets follow
  bool has_copy = false;
  uint8_t* copy_base = nullptr;
  int64_t copy_ls = 0, copy_limit = INT64_MAX;
  std::vector<int64_t> offs;
  std::vector<uint16_t> logs, mix;   // pre ++ post multiplier logs; mixing tables, rows of 8
  size_t n_pre = 0;
  std::vector<int> in_sd, out_sd;
};

// Plan `sp` (with `originals` of its K originals present, not all of them, and copy_present set
// by the caller's rule) as a job of a batch launch; bb.eligible stays false when it cannot be one.
void plan_batch_spec(const DecodeSpec& sp, uint32_t originals, BatchBlob& bb) {
  PlannedJob pj;
  if (plan_decode(sp, pj) != RS2_OK) return;  // the per-blob path reports it
  const bool fused = sp.copy_present && copy_covered(pj);
  if (!batch_eligible(pj, fused) || (originals > 0 && !fused)) return;
  bb.n_off = finish_plan(pj);
  pack_batch_job(pj, bb.job, bb.mix);
  bb.C = pj.C;
  bb.ppw = pj.ppw;
  bb.has_copy = !pj.copy_offs.empty();
  bb.copy_base = pj.copy_base;
  bb.copy_ls = pj.copy_ls;
  bb.copy_limit = pj.copy_limit;
  bb.offs = std::move(pj.offs);
  bb.n_pre = pj.pre_logs.size();
  bb.logs = std::move(pj.pre_logs);
  bb.logs.insert(bb.logs.end(), pj.post_logs.begin(), pj.post_logs.end());
  bb.in_sd = std::move(pj.in_sd);
  bb.out_sd = std::move(pj.out_sd);
  bb.eligible = true;
}

void plan_batch_blob(const rs2_plan* p, int axis, const BatchItem& it, const uint8_t* base,
                     BatchBlob& bb) {
  DecodeSpec sp;
  std::vector<int64_t> key;
  blob_decode_spec(p, axis, it.chosen, base, it.off, it.out, it.len, sp, key);
  uint32_t originals = 0;
  for (uint32_t i = 0; i < sp.K; ++i) originals += sp.present[i] >= 0;
  if (originals == sp.K) return;  // nothing erased: a copy (the per-blob path)
  sp.copy_present = originals > 0 && sp.symbol_size >= 4 && decode_may_fuse();
  plan_batch_spec(sp, originals, bb);
}

// Upload through the slot ring in pieces of at most a slot (never the runtime's copy from
// pageable memory, which Context::upload falls back to above a slot).
int upload_pieces(Context* ctx, void* dst, const void* src, size_t n, hipStream_t st) {
  for (size_t o = 0; o < n; o += UploadSlots::kSlotBytes)
    HIP_TRY(ctx->upload(static_cast<uint8_t*>(dst) + o, static_cast<const uint8_t*>(src) + o,
                        std::min(UploadSlots::kSlotBytes, n - o), st));
  return RS2_OK;
}

hipError_t launch_decode_batch(int C, const CodecJobBatch* d_jobs, int n_blobs, int tiles_per_blob,
                               int n_z, hipStream_t st) {
  switch (C) {
    case 1: return rs2k_launch_decode_batch_1(d_jobs, n_blobs, tiles_per_blob, n_z, st);
    case 2: return rs2k_launch_decode_batch_2(d_jobs, n_blobs, tiles_per_blob, n_z, st);
    case 4: return rs2k_launch_decode_batch_4(d_jobs, n_blobs, tiles_per_blob, n_z, st);
    case 8: return rs2k_launch_decode_batch_8(d_jobs, n_blobs, tiles_per_blob, n_z, st);
    case 16: return rs2k_launch_decode_batch_16(d_jobs, n_blobs, tiles_per_blob, n_z, st);
    case 32: return rs2k_launch_decode_batch_32(d_jobs, n_blobs, tiles_per_blob, n_z, st);
    case 64: return rs2k_launch_decode_batch_64(d_jobs, n_blobs, tiles_per_blob, n_z, st);
    case 128: return rs2k_launch_decode_batch_128(d_jobs, n_blobs, tiles_per_blob, n_z, st);
    case 256: return rs2k_launch_decode_batch_256(d_jobs, n_blobs, tiles_per_blob, n_z, st);
    case 512: return rs2k_launch_decode_batch_512(d_jobs, n_blobs, tiles_per_blob, n_z, st);
    default: return hipErrorInvalidValue;
  }
}

// What a window of a batched call runs with: its owner's (a blob plan's, a verifier's) slot pair,
// cursor, lines per job, profiler and planning stage name, and counters: launches, batched, single.
struct BatchRun {
  Context* ctx;
  BatchDecodeSlot (&slots)[2];
  int& cursor;
  int lines;
  Prof* prof;
  const char* plan_stage;
  std::atomic<uint64_t>&launches, &batched, &single;
};

hipError_t launch_decode_ranges(int C, const CodecJobBatch* d_jobs, const uint32_t* d_tiles,
                                int n_jobs, int n_tiles, int n_z, hipStream_t st) {
  switch (C) {
#define RS2_RANGES_CASE(CC) \
  case CC: return rs2k_launch_decode_ranges_##CC(d_jobs, d_tiles, n_jobs, n_tiles, n_z, st);
    RS2_RANGES_CASE(1)
    RS2_RANGES_CASE(2)
    RS2_RANGES_CASE(4)
    RS2_RANGES_CASE(8)
    RS2_RANGES_CASE(16)
    RS2_RANGES_CASE(32)
    RS2_RANGES_CASE(64)
    RS2_RANGES_CASE(128)
    RS2_RANGES_CASE(256)
    RS2_RANGES_CASE(512)
#undef RS2_RANGES_CASE
    default: return hipErrorInvalidValue;
  }
}

// One chunk: the blobs' arrays concatenated into the slot's device arrays, every job pointed
// at its own part, one table build over all the logs, one launch.  tiles null: every job has the
// tiles of the first one (cut_batch_chunks).  Else the chunk's tile prefix array
// (cut_range_chunks: a tile range per job); it goes up behind the job table.
int launch_batch_chunk(const BatchRun& run, std::vector<BatchBlob*>& ch, hipStream_t st,
                       const std::vector<uint32_t>* tiles = nullptr) {
  Context* ctx = run.ctx;
  BatchDecodeSlot& sl = run.slots[run.cursor];
  run.cursor ^= 1;
  HIP_TRY(sl.done.sync());
  if (run.prof) mark(run.prof, "", st);
  size_t n_offs = 0, n_logs = 0, n_mix = 0;
  for (const BatchBlob* bb : ch) {
    n_offs += bb->offs.size();
    n_logs += bb->logs.size();
    n_mix += bb->mix.size();
  }
  std::vector<int64_t> h_offs;
  std::vector<uint16_t> h_logs, h_mix;
  std::vector<CodecJobBatch> h_jobs;
  h_offs.reserve(n_offs);
  h_logs.reserve(n_logs);
  h_mix.reserve(n_mix);
  h_jobs.reserve(ch.size());
  HIP_TRY(sl.offs.ensure(std::max<size_t>(n_offs * 8, 16)));
  HIP_TRY(sl.logs.ensure(std::max<size_t>(n_logs * 2, 16)));
  HIP_TRY(sl.tabs.ensure(std::max<size_t>(n_logs * kTabU16 * 2, 16)));
  HIP_TRY(sl.mix.ensure(std::max<size_t>(n_mix * 2, 16)));
  static_assert(sizeof(CodecJobBatch) % 4 == 0, "the tile prefix array follows the job table");
  const size_t jobs_b = ch.size() * sizeof(CodecJobBatch);
  HIP_TRY(sl.jobs.ensure(jobs_b + (tiles ? tiles->size() * 4 : 0)));
  const int C = ch[0]->C;
  const int64_t per_blob = (int64_t(run.lines) * ch[0]->job.pairs_span + 63) / 64;
  if (tiles ? tiles->size() != ch.size() + 1
            : per_blob < 1 || per_blob * int64_t(ch.size()) > 0x7FFFFFFF)
    return fail(RS2_E_UNSUPPORTED, "decode batch chunk exceeds the launch grid");
  int n_z = 1;
  for (BatchBlob* bb : ch) {
    CodecJobBatch j = bb->job;
    const int64_t* d_offs = sl.offs.as<int64_t>() + h_offs.size();
    const uint16_t* d_tabs = sl.tabs.as<uint16_t>() + h_logs.size() * kTabU16;
    for (int b = 0; b < j.n_in; ++b) {
      InBlock& ib = j.in[b];
      ib.pos_off = d_offs + size_t(b) * bb->C;
      if (bb->has_copy) {
        ib.copy_base = bb->copy_base;
        ib.copy_off = d_offs + bb->n_off + size_t(b) * bb->C;
        ib.copy_line_stride = bb->copy_ls;
        ib.copy_limit = bb->copy_limit;
      } else {
        ib.copy_off = nullptr;
      }
      ib.sd_tab = ctx->stream(bb->C, bb->in_sd[size_t(b)], bb->ppw);
      if (!ib.sd_tab) return fail(RS2_E_DEVICE, "table upload failed");
      ib.zero_first = group0_zero(bb->C, bb->in_sd[size_t(b)], bb->ppw);
      ib.pre_tab = d_tabs + size_t(b) * bb->C * kTabU16;
    }
    j.pre_z_stride = int64_t(j.n_in) * bb->C * kTabU16;
    for (int o = 0; o < j.n_out; ++o) {
      OutBlock& ob = j.out[o];
      ob.pos_off = d_offs + size_t(j.n_in + o) * bb->C;
      ob.sd_tab = ctx->stream(bb->C, bb->out_sd[size_t(o)], bb->ppw);
      if (!ob.sd_tab) return fail(RS2_E_DEVICE, "table upload failed");
      ob.zero_first = group0_zero(bb->C, bb->out_sd[size_t(o)], bb->ppw);
      ob.post_tab = d_tabs + (bb->n_pre + size_t(o) * bb->C) * kTabU16;
    }
    j.mix_tab = bb->mix.empty() ? nullptr : sl.mix.as<uint16_t>() + h_mix.size();
    // the launch's fields (set_launch_shape): this blob alone, lines folded into the tiles
    j.n_lines = run.lines;
    j.line_base = 0;
    j.tiles_per_blob = 0;
    j.in_blob_stride = j.out_blob_stride = j.copy_blob_stride = 0;
    j.stamps = nullptr;
    j.tile_ctr = nullptr;
    n_z = std::max(n_z, j.n_out);
    h_jobs.push_back(j);
    h_offs.insert(h_offs.end(), bb->offs.begin(), bb->offs.end());
    h_logs.insert(h_logs.end(), bb->logs.begin(), bb->logs.end());
    h_mix.insert(h_mix.end(), bb->mix.begin(), bb->mix.end());
  }
  RS2_TRY(upload_pieces(ctx, sl.offs.p, h_offs.data(), h_offs.size() * 8, st));
  RS2_TRY(upload_pieces(ctx, sl.logs.p, h_logs.data(), h_logs.size() * 2, st));
  RS2_TRY(upload_pieces(ctx, sl.mix.p, h_mix.data(), h_mix.size() * 2, st));
  RS2_TRY(upload_pieces(ctx, sl.jobs.p, h_jobs.data(), jobs_b, st));
  if (tiles)
    RS2_TRY(upload_pieces(ctx, sl.jobs.as<uint8_t>() + jobs_b, tiles->data(), tiles->size() * 4, st));
  HIP_TRY(rs2k_launch_build_mul_tables(ctx->exp_t.as<uint16_t>(), ctx->log_t.as<uint16_t>(),
                                       sl.logs.as<uint16_t>(), int(h_logs.size()),
                                       sl.tabs.as<uint16_t>(), st));
  if (run.prof) mark(run.prof, "dec_batch_setup", st);
  if (tiles)
    HIP_TRY(launch_decode_ranges(
        C, sl.jobs.as<CodecJobBatch>(), reinterpret_cast<const uint32_t*>(sl.jobs.as<uint8_t>() + jobs_b),
        int(ch.size()), int(tiles->back()), n_z, st));
  else
    HIP_TRY(launch_decode_batch(C, sl.jobs.as<CodecJobBatch>(), int(ch.size()), int(per_blob), n_z,
                                st));
  if (run.prof) mark(run.prof, "dec_batch_codec", st);
  HIP_TRY(sl.done.record(st));
  return RS2_OK;
}

// One window of cnt items: plan(i, job) for every item on the host pool; the eligible jobs in
// chunks (cut_batch_chunks within kBatchTableBytes), one launch each on st; every other item,
// those the cut demotes included, through single(i) on the same stream.
template <class Plan, class Single>
int run_batch_window(const BatchRun& run, size_t cnt, hipStream_t st, Plan plan, Single single) {
  std::vector<BatchBlob> jobs(cnt);
  const auto host_t0 = std::chrono::steady_clock::now();
  pool_for_each(run.ctx->pool, cnt, [&](size_t i) { plan(i, jobs[i]); });
  prof_host(run.prof, run.plan_stage, host_t0);
  std::vector<ChunkJob> geo(cnt);
  for (size_t i = 0; i < cnt; ++i)
    geo[i] = {jobs[i].eligible, jobs[i].C, jobs[i].job.pairs_span, jobs[i].logs.size()};
  ChunkCut cut;
  cut_batch_chunks(geo, kBatchTableBytes, cut);
  for (uint32_t i : cut.demoted) jobs[i].eligible = false;
  std::vector<BatchBlob*> ch;
  for (size_t c = 0, at = 0; c < cut.ends.size(); at = cut.ends[c++]) {
    ch.clear();
    for (size_t m = at; m < cut.ends[c]; ++m) ch.push_back(&jobs[cut.members[m]]);
    RS2_TRY(launch_batch_chunk(run, ch, st));
    run.launches.fetch_add(1, std::memory_order_relaxed);
    run.batched.fetch_add(ch.size(), std::memory_order_relaxed);
  }
  for (size_t i = 0; i < cnt; ++i) {
    if (jobs[i].eligible) continue;
    RS2_TRY(single(i));
    run.single.fetch_add(1, std::memory_order_relaxed);
  }
  return RS2_OK;
}

// Decode validated blobs: windows of at most a chunk's jobs are planned on the host pool, the
// eligible blobs of a window leave in chunks (one launch each), the others through the
// per-blob decode on the same stream.
int decode_batch_items(rs2_plan* p, int axis, const std::vector<BatchItem>& items,
                       const uint8_t* base, hipStream_t st) {
  const int lines = axis == RS2_AXIS_PRIMARY ? int(p->ks) : int(p->kp);
  const BatchRun run{p->ctx, p->dbatch, p->dbatch_slot, lines, &p->prof, "dec_batch_plan_host",
                     g_batch_launches, g_batch_blobs, g_batch_single};
  for (size_t w0 = 0; w0 < items.size(); w0 += kBatchChunkJobs) {
    const size_t cnt = std::min(kBatchChunkJobs, items.size() - w0);
    RS2_TRY(run_batch_window(
        run, cnt, st,
        [&](size_t i, BatchBlob& bb) { plan_batch_blob(p, axis, items[w0 + i], base, bb); },
        [&](size_t i) {
          const BatchItem& it = items[w0 + i];
          return decode_device(p, axis, it.chosen, base, it.off, it.out, st, it.len);
        }));
  }
  return RS2_OK;
}

// Per-blob length rule of the batch calls: blob_lens[b] (NULL: the plan's) gives the plan's
// symbol size.
int batch_blob_len(const rs2_plan* p, const uint64_t* blob_lens, uint32_t b, uint64_t* len) {
  *len = blob_lens ? blob_lens[b] : p->blob_len;
  uint16_t sb = 0;
  if (rs2_symbol_size_for_blob(p->n, *len, &sb) != RS2_OK || sb != p->s)
    return fail(RS2_E_INVALID_ARGUMENT, "blob length outside the plan's symbol size");
  return RS2_OK;
}

// The per-blob rules of the device batch calls (rs2_decode_batch_device_async and its verified
// form) for every blob: the accepted blobs in `items`, in slot order.  status_out NULL: the first
// failing blob's code is returned; non-NULL: every blob's code is stored, RS2_OK.
int validate_batch_device(const rs2_plan* plan, int axis, uint32_t n_blobs,
                          const uint64_t* blob_lens, const uint32_t* counts,
                          const uint16_t* sliver_idx, const uint64_t* sliver_off,
                          void* d_blobs_out, uint64_t out_stride, int* status_out,
                          std::vector<BatchItem>& items) {
  items.clear();
  items.reserve(n_blobs);
  size_t first = 0;
  for (uint32_t b = 0; b < n_blobs; first += counts[b], ++b) {
    BatchItem it;
    it.blob = b;
    it.off = sliver_off + first;
    it.idx = sliver_idx + first;
    it.out = reinterpret_cast<uint8_t*>(d_blobs_out) + uint64_t(b) * out_stride;
    auto validate = [&]() -> int {
      RS2_TRY(batch_blob_len(plan, blob_lens, b, &it.len));
      if (n_blobs > 1 && it.len > out_stride)
        return fail(RS2_E_INVALID_ARGUMENT, "out_stride smaller than a blob");
      for (uint32_t i = 0; i < counts[b]; ++i)
        RS2_TRY(check_symbol_step(it.off[i], "sliver_off[i]"));
      return select_slivers(plan, axis, counts[b], it.idx, nullptr, nullptr, it.chosen,
                            &it.pulled);
    };
    bool ok;
    RS2_TRY(slot_outcome(validate(), status_out, b, &ok));
    if (ok) items.push_back(std::move(it));
  }
  return RS2_OK;
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

int rs2_source_symbols_for_n_shards(uint16_t n_shards, uint16_t* n_primary, uint16_t* n_secondary) {
  if (n_shards == 0 || !n_primary || !n_secondary)
    return fail(RS2_E_INVALID_ARGUMENT, "n_shards must be non-zero");
  const uint16_t f = uint16_t((n_shards - 1) / 3);
  *n_secondary = uint16_t(n_shards - f);
  *n_primary = uint16_t(n_shards - 2 * f);
  return RS2_OK;
}

int rs2_symbol_size_for_blob(uint16_t n_shards, uint64_t blob_len, uint16_t* symbol_size) {
  uint16_t kp, ks;
  RS2_TRY(rs2_source_symbols_for_n_shards(n_shards, &kp, &ks));
  const uint64_t n_sym = uint64_t(kp) * ks;
  const uint64_t len = std::max<uint64_t>(blob_len, 1);
  uint64_t sz = (len + n_sym - 1) / n_sym;
  sz = (sz + 1) / 2 * 2;
  if (sz > 0xFFFF) return fail(RS2_E_DATA_TOO_LARGE, "blob too large for the symbol size");
  *symbol_size = uint16_t(sz);
  return RS2_OK;
}

int rs2_encoded_blob_length(uint16_t n_shards, uint64_t blob_len, uint64_t* encoded_len) {
  uint16_t kp, ks, s;
  RS2_TRY(rs2_source_symbols_for_n_shards(n_shards, &kp, &ks));
  RS2_TRY(rs2_symbol_size_for_blob(n_shards, blob_len, &s));
  const uint64_t slivers = uint64_t(n_shards) * (uint64_t(kp) + ks) * s;
  const uint64_t meta = uint64_t(n_shards) * (uint64_t(n_shards) * 64 + 32);
  *encoded_len = slivers + meta;
  return RS2_OK;
}

int rs2_set_device(int device) {
  g_device = device;
  return RS2_OK;
}

const char* rs2_last_error(void) { return last_error(); }

int rs2_device_available(void) {
  int n = 0;
  return (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? 1 : 0;
}

int rs2_set_block_limit(uint32_t max_block) {
  if (max_block < 1 || max_block > uint32_t(kMaxC) || (max_block & (max_block - 1)))
    return fail(RS2_E_INVALID_ARGUMENT, "block limit must be a power of two <= 512");
  set_block_max(max_block);
  return RS2_OK;
}

int rs2_plan_create(uint16_t n_shards, uint64_t blob_len, rs2_plan** out) {
  if (!out) return fail(RS2_E_INVALID_ARGUMENT, "null plan pointer");
  *out = nullptr;
  uint16_t kp, ks, s;
  RS2_TRY(rs2_source_symbols_for_n_shards(n_shards, &kp, &ks));
  RS2_TRY(rs2_symbol_size_for_blob(n_shards, blob_len, &s));
  if (kp == n_shards || ks == n_shards)
    return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "n_shards too small for a recovery code");
  if (n_shards > kMaxShards) return fail(RS2_E_UNSUPPORTED, "n_shards above 65535");
  Context* ctx = nullptr;
  RS2_TRY(get_context(&ctx));
  auto p = std::make_unique<rs2_plan>();
  p->ctx = ctx;
  p->n = n_shards;
  p->kp = kp;
  p->ks = ks;
  p->s = s;
  p->blob_len = blob_len;
  HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  HIP_TRY(hipStreamCreateWithFlags(&p->side, hipStreamNonBlocking));
  const int64_t n = n_shards;
  HIP_TRY(p->both.ensure(size_t(n - kp) * (n - ks) * s));
  HIP_TRY(p->leaves.ensure(size_t(n) * n * 32));
  HIP_TRY(p->pairs.ensure(size_t(n) * 64));
  HIP_TRY(p->blob_id.ensure(32));
  // systematic secondary copy offsets: a = column c
  std::vector<int64_t> sa(ks), da(ks);
  for (int64_t c = 0; c < ks; ++c) {
    sa[c] = c * s;
    da[c] = c * kp * s;
  }
  HIP_TRY(p->sys_a_src.ensure(sa.size() * 8));
  HIP_TRY(p->sys_a_dst.ensure(da.size() * 8));
  HIP_TRY(hipMemcpy(p->sys_a_src.p, sa.data(), sa.size() * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(p->sys_a_dst.p, da.data(), da.size() * 8, hipMemcpyHostToDevice));
  *out = p.release();
  return RS2_OK;
}

int rs2_plan_info_get(const rs2_plan* plan, rs2_plan_info* info) {
  if (!plan || !info) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  info->n_shards = plan->n;
  info->n_primary = plan->kp;
  info->n_secondary = plan->ks;
  info->symbol_size = plan->s;
  info->blob_len = plan->blob_len;
  info->primary_sliver_len = uint64_t(primary_len(plan));
  info->secondary_sliver_len = uint64_t(secondary_len(plan));
  return RS2_OK;
}

void rs2_plan_destroy(rs2_plan* plan) {
  if (!plan) return;
  (void)hipSetDevice(plan->ctx->device);
  // every stream and event the plan's work may still run behind (no device-wide synchronize):
  // its buffers then go straight back to the device arena for the next plan
  for (hipStream_t st : {plan->stream, plan->side, plan->side_hi, plan->aux, plan->io})
    if (st) (void)hipStreamSynchronize(st);
  for (const Event* ev : {&plan->enc_done, &plan->dec[0].done, &plan->dec[1].done, &plan->leaf_ev,
                          &plan->dbatch[0].done, &plan->dbatch[1].done, &plan->vb_done})
    (void)ev->sync();
  const Quiesced quiesced;
  delete plan;
}

int rs2_plan_rebind(rs2_plan* plan, uint64_t blob_len) {
  if (!plan) return fail(RS2_E_INVALID_ARGUMENT, "null plan");
  uint16_t s = 0;
  RS2_TRY(rs2_symbol_size_for_blob(plan->n, blob_len, &s));
  if (s != plan->s)
    return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "blob length needs another symbol size than the plan's");
  plan->blob_len = blob_len;
  return RS2_OK;
}

int rs2_host_register(void* ptr, uint64_t len) {
  if (!ptr || !len) return fail(RS2_E_INVALID_ARGUMENT, "null or empty range");
  const uintptr_t p = reinterpret_cast<uintptr_t>(ptr);
  std::lock_guard<std::mutex> lk(g_reg_mu);
  auto it = g_reg.lower_bound(p);
  if (it != g_reg.end() && it->first < p + len)
    return fail(RS2_E_INVALID_ARGUMENT, "range overlaps a registered range");
  if (it != g_reg.begin() && std::prev(it)->first + std::prev(it)->second > p)
    return fail(RS2_E_INVALID_ARGUMENT, "range overlaps a registered range");
  HIP_TRY(hipHostRegister(ptr, size_t(len), hipHostRegisterPortable));
  g_reg.emplace(p, size_t(len));
  return RS2_OK;
}

int rs2_host_unregister(void* ptr) {
  std::lock_guard<std::mutex> lk(g_reg_mu);
  auto it = g_reg.find(reinterpret_cast<uintptr_t>(ptr));
  if (it == g_reg.end()) return fail(RS2_E_INVALID_ARGUMENT, "pointer was not registered");
  g_reg.erase(it);
  HIP_TRY(hipHostUnregister(ptr));
  return RS2_OK;
}

int rs2_device_memory_stats(int device, uint64_t* stats_out) {
  if (!stats_out) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  DevArena& a = dev_arena(device);
  std::lock_guard<std::mutex> lk(a.mu);
  stats_out[0] = a.mallocs;
  stats_out[1] = a.frees;
  stats_out[2] = uint64_t(a.live);
  stats_out[3] = a.reserved;
  stats_out[4] = uint64_t(a.peak);
  stats_out[5] = a.syncs;
  stats_out[6] = g_pinned_allocs.load(std::memory_order_relaxed);
  return RS2_OK;
}

int rs2_upload_stats(uint64_t* stats_out) {
  return read_stats(stats_out, {&g_upload_calls, &g_upload_jobs, &g_upload_waits});
}

int rs2_device_memory_trim(int device, uint64_t* released_bytes) {
  if (released_bytes) *released_bytes = 0;
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(RS2_E_INVALID_ARGUMENT, "bad device");
  int prev = 0;
  HIP_TRY(hipGetDevice(&prev));
  HIP_TRY(hipSetDevice(device));
  const hipError_t e = dev_arena(device).trim(released_bytes);
  (void)hipSetDevice(prev);
  HIP_TRY(e);
  return RS2_OK;
}

int rs2_encode_device_async(rs2_plan* plan, const void* d_blob, void* d_primary, void* d_secondary,
                            void* d_hashes, void* d_blob_id, void* stream) {
  if (!plan || !d_primary || !d_secondary || (!d_blob && plan->blob_len))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  RS2_TRY(check_encode_ptrs(d_blob, d_primary, d_secondary, d_hashes, d_blob_id));
  HIP_TRY(hipSetDevice(plan->ctx->device));
  return encode_device(plan, reinterpret_cast<const uint8_t*>(d_blob),
                       reinterpret_cast<uint8_t*>(d_primary), reinterpret_cast<uint8_t*>(d_secondary),
                       reinterpret_cast<uint8_t*>(d_hashes), reinterpret_cast<uint8_t*>(d_blob_id),
                       pick_stream(plan, stream), true);
}

int rs2_compute_metadata_device_async(rs2_plan* plan, const void* d_blob, void* d_hashes,
                                      void* d_blob_id, void* stream) {
  if (!plan || !d_hashes || !d_blob_id || (!d_blob && plan->blob_len))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  RS2_TRY(check_encode_ptrs(d_blob, nullptr, nullptr, d_hashes, d_blob_id));
  HIP_TRY(hipSetDevice(plan->ctx->device));
  return encode_metadata(plan, reinterpret_cast<const uint8_t*>(d_blob),
                         reinterpret_cast<uint8_t*>(d_hashes), reinterpret_cast<uint8_t*>(d_blob_id),
                         pick_stream(plan, stream));
}

int rs2_encode_device_split_async(rs2_plan* plan, const void* d_blob, void* d_primary,
                                  void* d_secondary, void* d_hashes, void* d_blob_id, void* stream,
                                  void* primary_stream) {
  if (!plan || !d_primary || !d_secondary || (!d_blob && plan->blob_len) || !primary_stream)
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  RS2_TRY(check_encode_ptrs(d_blob, d_primary, d_secondary, d_hashes, d_blob_id));
  hipStream_t st = pick_stream(plan, stream);
  hipStream_t pst = abi_stream(primary_stream, nullptr);
  if (pst == st || pst == plan->side || pst == plan->side_hi)
    return fail(RS2_E_INVALID_ARGUMENT, "primary_stream must differ from stream");
  HIP_TRY(hipSetDevice(plan->ctx->device));
  return encode_device(plan, reinterpret_cast<const uint8_t*>(d_blob),
                       reinterpret_cast<uint8_t*>(d_primary), reinterpret_cast<uint8_t*>(d_secondary),
                       reinterpret_cast<uint8_t*>(d_hashes), reinterpret_cast<uint8_t*>(d_blob_id),
                       st, true, pst);
}

int rs2_decode_device_async(rs2_plan* plan, int axis, uint32_t count, const uint16_t* sliver_idx,
                            const void* d_slivers_base, const uint64_t* sliver_off,
                            void* d_blob_out, void* stream) {
  if (!plan || !sliver_idx || !sliver_off || !d_slivers_base || !d_blob_out)
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  RS2_TRY(check_axis(axis));
  RS2_TRY(check_decode_ptrs(count, d_slivers_base, sliver_off, d_blob_out));
  HIP_TRY(hipSetDevice(plan->ctx->device));
  std::vector<std::pair<uint16_t, uint32_t>> chosen;
  RS2_TRY(select_slivers(plan, axis, count, sliver_idx, nullptr, nullptr, chosen));
  return decode_device(plan, axis, chosen, reinterpret_cast<const uint8_t*>(d_slivers_base),
                       sliver_off, reinterpret_cast<uint8_t*>(d_blob_out), pick_stream(plan, stream),
                       plan->blob_len);
}

int rs2_profile_enable(rs2_plan* plan, int enable) {
  if (!plan) return fail(RS2_E_INVALID_ARGUMENT, "null plan");
  plan->prof.on = enable != 0;
  return RS2_OK;
}

int rs2_profile_read(rs2_plan* plan, uint32_t max_stages, char* names, double* total_ms,
                     uint32_t* launches, uint32_t* n_stages) {
  if (!plan || !n_stages) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  (void)hipSetDevice(plan->ctx->device);
  return prof_read(plan->prof, max_stages, names, total_ms, launches, n_stages);
}

int rs2_verifier_profile_enable(rs2_verifier* v, int enable) {
  if (!v) return fail(RS2_E_INVALID_ARGUMENT, "null verifier");
  v->prof.on = enable != 0;
  return RS2_OK;
}

int rs2_verifier_profile_read(rs2_verifier* v, uint32_t max_stages, char* names, double* total_ms,
                              uint32_t* launches, uint32_t* n_stages) {
  if (!v || !n_stages) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  (void)hipSetDevice(v->ctx->device);
  return prof_read(v->prof, max_stages, names, total_ms, launches, n_stages);
}

int rs2_sync(rs2_plan* plan, void* stream) {
  if (!plan) return fail(RS2_E_INVALID_ARGUMENT, "null plan");
  HIP_TRY(hipStreamSynchronize(pick_stream(plan, stream)));
  return RS2_OK;
}

}  // extern "C"

namespace {
// a pinned ring leased to `plan` for one host-buffer call
struct RingGuard {
  rs2_plan* p;
  StagerLease lease;
  explicit RingGuard(rs2_plan* plan) : p(plan), lease(plan->ctx->device) { p->stage = lease.st.get(); }
  ~RingGuard() {
    // the ring's slot events were recorded on this plan's streams, which may be destroyed before
    // the next lease waits on them: drain them and move them to the context's stream
    for (Event& ev : lease.st->ev)
      if (ev.set()) {
        (void)ev.sync();
        (void)ev.record(p->ctx->util_stream);
      }
    p->stage = nullptr;
  }
};
}  // namespace

extern "C" {

int rs2_encode_with_metadata(rs2_plan* plan, const uint8_t* blob, uint8_t* const* primary_out,
                             uint8_t* const* secondary_out, uint8_t* hashes_out,
                             uint8_t* blob_id_out) {
  if (!plan || (!blob && plan->blob_len)) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(plan->ctx->device));
  RingGuard ring(plan);
  Context* ctx = plan->ctx;
  const int64_t n = plan->n, pl = primary_len(plan), sl = secondary_len(plan);
  // the message size (not blob_len): a plan rebound to another length of its symbol size keeps it
  HIP_TRY(plan->dev_blob.ensure(std::max<uint64_t>(uint64_t(plan->kp) * plan->ks * plan->s, 16)));
  HIP_TRY(plan->int_primary.ensure(size_t(n) * pl));
  HIP_TRY(plan->int_secondary.ensure(size_t(n) * sl));
  if (!plan->io) HIP_TRY(hipStreamCreateWithFlags(&plan->io, hipStreamNonBlocking));
  hipStream_t st = plan->stream, io = plan->io;
  // the blob in through the pinned ring (host copies of piece k+1 under the DMA of piece k)
  if (plan->blob_len)
    RS2_TRY(stage_h2d(ctx, *plan->stage, {{const_cast<uint8_t*>(blob), plan->dev_blob.as<uint8_t>(),
                                           size_t(plan->blob_len)}}, st));
  uint8_t* dp = plan->int_primary.as<uint8_t>();
  uint8_t* ds = plan->int_secondary.as<uint8_t>();
  const bool slivers = primary_out || secondary_out;
  // split encode: `io` is released once the primary slivers are final, so their D2H overlaps the
  // secondary codecs and the hashing still running on st
  RS2_TRY(encode_device(plan, plan->dev_blob.as<uint8_t>(), dp, ds, plan->pairs.as<uint8_t>(),
                        plan->blob_id.as<uint8_t>(), st, slivers, slivers ? io : nullptr));
  std::vector<Seg> segs;
  for (int64_t i = 0; primary_out && i < n; ++i)
    if (primary_out[i]) segs.push_back({primary_out[i], dp + i * pl, size_t(pl)});
  if (!segs.empty()) RS2_TRY(stage_d2h(ctx, *plan->stage, segs, io));
  segs.clear();
  for (int64_t i = 0; secondary_out && i < n; ++i)
    if (secondary_out[i]) segs.push_back({secondary_out[i], ds + i * sl, size_t(sl)});
  if (hashes_out) segs.push_back({hashes_out, plan->pairs.as<uint8_t>(), size_t(n) * 64});
  if (blob_id_out) segs.push_back({blob_id_out, plan->blob_id.as<uint8_t>(), 32});
  HIP_TRY(plan->enc_done.wait_on(io));
  if (!segs.empty()) RS2_TRY(stage_d2h(ctx, *plan->stage, segs, io));
  HIP_TRY(hipStreamSynchronize(io));
  HIP_TRY(hipStreamSynchronize(st));
  return RS2_OK;
}

int rs2_compute_metadata(rs2_plan* plan, const uint8_t* blob, uint8_t* hashes_out,
                         uint8_t* blob_id_out) {
  return rs2_encode_with_metadata(plan, blob, nullptr, nullptr, hashes_out, blob_id_out);
}

int rs2_encode_batch_device_async(rs2_plan* plan, uint32_t n_blobs, const void* d_blobs,
                                  uint64_t blob_stride, const uint64_t* blob_lens, void* d_primary,
                                  uint64_t primary_stride, void* d_secondary,
                                  uint64_t secondary_stride, void* d_hashes, void* d_blob_ids,
                                  void* stream) {
  if (!plan) return fail(RS2_E_INVALID_ARGUMENT, "null plan");
  RS2_TRY(check_encode_ptrs(d_blobs, d_primary, d_secondary, d_hashes, d_blob_ids));
  RS2_TRY(check_symbol_step(blob_stride, "blob_stride"));
  RS2_TRY(check_symbol_step(primary_stride, "primary_stride"));
  RS2_TRY(check_symbol_step(secondary_stride, "secondary_stride"));
  HIP_TRY(hipSetDevice(plan->ctx->device));
  return encode_batch_device(plan, n_blobs, reinterpret_cast<const uint8_t*>(d_blobs),
                             int64_t(blob_stride), blob_lens, reinterpret_cast<uint8_t*>(d_primary),
                             int64_t(primary_stride), reinterpret_cast<uint8_t*>(d_secondary),
                             int64_t(secondary_stride), reinterpret_cast<uint8_t*>(d_hashes),
                             reinterpret_cast<uint8_t*>(d_blob_ids), pick_stream(plan, stream));
}

int rs2_encode_batch_with_metadata(rs2_plan* plan, uint32_t n_blobs, const uint8_t* const* blobs,
                                   const uint64_t* blob_lens, uint8_t* const* primary_out,
                                   uint8_t* const* secondary_out, uint8_t* hashes_out,
                                   uint8_t* blob_ids_out) {
  if (!plan) return fail(RS2_E_INVALID_ARGUMENT, "null plan");
  bool empty;
  RS2_TRY(batch_count(n_blobs, "blobs in a batch", true, &empty));
  if (empty) return RS2_OK;
  HIP_TRY(hipSetDevice(plan->ctx->device));
  RingGuard ring(plan);
  Context* ctx = plan->ctx;
  const int64_t n = plan->n, pl = primary_len(plan), sl = secondary_len(plan);
  const size_t B = n_blobs;
  uint64_t max_len = 0;
  for (size_t b = 0; b < B; ++b) {
    const uint64_t len = blob_lens ? blob_lens[b] : plan->blob_len;
    if (len && (!blobs || !blobs[b])) return fail(RS2_E_INVALID_ARGUMENT, "null blob");
    max_len = std::max(max_len, len);
  }
  const int64_t bstride = int64_t((std::max<uint64_t>(max_len, 1) + 255) / 256 * 256);
  HIP_TRY(plan->batch_blob.ensure(B * size_t(bstride)));
  HIP_TRY(plan->batch_primary.ensure(B * size_t(n * pl)));
  HIP_TRY(plan->batch_secondary.ensure(B * size_t(n * sl)));
  HIP_TRY(plan->batch_hashes.ensure(B * size_t(n) * 64));
  HIP_TRY(plan->batch_ids.ensure(B * 32));
  hipStream_t st = plan->stream;
  uint8_t* db = plan->batch_blob.as<uint8_t>();
  uint8_t* dp = plan->batch_primary.as<uint8_t>();
  uint8_t* ds = plan->batch_secondary.as<uint8_t>();
  uint8_t* dh = plan->batch_hashes.as<uint8_t>();
  uint8_t* di = plan->batch_ids.as<uint8_t>();
  std::vector<Seg> segs;
  for (size_t b = 0; b < B; ++b) {
    const uint64_t len = blob_lens ? blob_lens[b] : plan->blob_len;
    if (len) segs.push_back({const_cast<uint8_t*>(blobs[b]), db + b * bstride, size_t(len)});
  }
  RS2_TRY(stage_h2d(ctx, *plan->stage, segs, st));
  RS2_TRY(encode_batch_device(plan, n_blobs, db, bstride, blob_lens, dp, n * pl, ds, n * sl, dh, di, st));
  segs.clear();
  for (size_t b = 0; b < B; ++b)
    for (int64_t i = 0; i < n; ++i) {
      if (primary_out && primary_out[b * n + i])
        segs.push_back({primary_out[b * n + i], dp + (b * n + i) * pl, size_t(pl)});
      if (secondary_out && secondary_out[b * n + i])
        segs.push_back({secondary_out[b * n + i], ds + (b * n + i) * sl, size_t(sl)});
    }
  if (hashes_out) segs.push_back({hashes_out, dh, B * size_t(n) * 64});
  if (blob_ids_out) segs.push_back({blob_ids_out, di, B * 32});
  if (!segs.empty()) RS2_TRY(stage_d2h(ctx, *plan->stage, segs, st));
  HIP_TRY(hipStreamSynchronize(st));
  return RS2_OK;
}

int rs2_decode_batch_device_async(rs2_plan* plan, int axis, uint32_t n_blobs,
                                  const uint64_t* blob_lens, const uint32_t* counts,
                                  const uint16_t* sliver_idx, const void* d_slivers_base,
                                  const uint64_t* sliver_off, void* d_blobs_out,
                                  uint64_t out_stride, int* status_out, void* stream) {
  if (!plan) return fail(RS2_E_INVALID_ARGUMENT, "null plan");
  RS2_TRY(check_axis(axis));
  bool empty;
  RS2_TRY(batch_count(n_blobs, "blobs in a batch",
                      counts && sliver_idx && sliver_off && d_slivers_base && d_blobs_out, &empty));
  if (empty) return RS2_OK;
  RS2_TRY(check_symbol_ptr(d_slivers_base, "d_slivers_base"));
  RS2_TRY(check_symbol_ptr(d_blobs_out, "d_blobs_out"));
  RS2_TRY(check_symbol_step(out_stride, "out_stride"));
  HIP_TRY(hipSetDevice(plan->ctx->device));
  // every blob is validated before anything is enqueued
  std::vector<BatchItem> items;
  RS2_TRY(validate_batch_device(plan, axis, n_blobs, blob_lens, counts, sliver_idx, sliver_off,
                                d_blobs_out, out_stride, status_out, items));
  return decode_batch_items(plan, axis, items, reinterpret_cast<const uint8_t*>(d_slivers_base),
                            pick_stream(plan, stream));
}

int rs2_decode_batch_stats(uint64_t* stats_out) {
  return read_stats(stats_out, {&g_batch_launches, &g_batch_blobs, &g_batch_single});
}

}  // extern "C"

namespace {

// Host slivers -> decoded blob in plan->dev_blob (blob_len bytes, zero up to the K_p*K_s*s
// message size so its rows are the zero-padded systematic primary slivers), enqueued on the
// plan stream.  *pulled: input slivers consumed (select_slivers).
int decode_host(rs2_plan* plan, int axis, uint32_t count, const uint16_t* sliver_idx,
                const uint8_t* const* slivers, const uint64_t* sliver_len,
                const uint16_t* sliver_symbol_size, uint32_t* pulled) {
  if (count && (!sliver_idx || !slivers || !sliver_len))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  RS2_TRY(check_axis(axis));
  HIP_TRY(hipSetDevice(plan->ctx->device));
  std::vector<std::pair<uint16_t, uint32_t>> chosen;
  RS2_TRY(select_slivers(plan, axis, count, sliver_idx, sliver_len, sliver_symbol_size, chosen,
                         pulled));
  for (const auto& c : chosen)
    if (!slivers[c.second]) return fail(RS2_E_INVALID_ARGUMENT, "null sliver");
  const int64_t len = axis == RS2_AXIS_PRIMARY ? primary_len(plan) : secondary_len(plan);
  const int64_t msg = int64_t(plan->kp) * plan->ks * plan->s;
  hipStream_t st = plan->stream;
  // the chosen slivers, back to back on the device, through the pinned ring
  DevBuf& stage = axis == RS2_AXIS_PRIMARY ? plan->int_primary : plan->int_secondary;
  HIP_TRY(stage.ensure(size_t(plan->n) * len));  // the encoder's size: never re-allocated
  std::vector<uint64_t> off(count, 0);
  std::vector<Seg> segs;
  for (size_t i = 0; i < chosen.size(); ++i) {
    off[chosen[i].second] = uint64_t(i) * len;
    segs.push_back({const_cast<uint8_t*>(slivers[chosen[i].second]),
                    stage.as<uint8_t>() + i * len, size_t(len)});
  }
  HIP_TRY(plan->dev_blob.ensure(size_t(std::max<int64_t>(msg, 16))));
  RS2_TRY(stage_h2d(plan->ctx, *plan->stage, segs, st));
  if (uint64_t(msg) > plan->blob_len)
    HIP_TRY(hipMemsetAsync(plan->dev_blob.as<uint8_t>() + plan->blob_len, 0,
                           size_t(msg - plan->blob_len), st));
  return decode_device(plan, axis, chosen, stage.as<uint8_t>(), off.data(),
                       plan->dev_blob.as<uint8_t>(), st, plan->blob_len);
}

// Default consistency check (blob_encoding.rs:579-612) on a decoded blob on the device (`blob`,
// `blob_valid` bytes of it written: plan->dev_blob of the host path holds the whole zero-padded
// message, a caller's device buffer only blob_len bytes): every systematic primary sliver
// i < K_p not marked in `verified` is re-expanded with the secondary code, its n symbols
// leaf-hashed and Merkle-reduced on the device, and the root compared with the metadata's
// primary hash of pair i.
int default_check(rs2_plan* plan, const std::vector<uint8_t>& verified, const uint8_t* hashes,
                  const uint8_t* blob, int64_t blob_valid, hipStream_t st) {
  const int64_t kp = plan->kp, ks = plan->ks, s = plan->s, row = ks * s;
  std::vector<uint16_t> rows;
  for (int64_t i = 0; i < kp; ++i)
    if (!verified[size_t(i)]) rows.push_back(uint16_t(i));
  if (rows.empty()) return RS2_OK;
  if (!plan->check_v) {
    RS2_TRY(rs2_verifier_create(plan->n, plan->s, RS2_AXIS_PRIMARY, &plan->check_v));
  }
  const uint8_t* src = blob;
  // rows past the written bytes (the zero-padded tail of the message) are rebuilt in the gather
  // buffer: zeros, then the row's written prefix
  std::vector<size_t> partial;
  for (size_t a = 0; a < rows.size(); ++a)
    if (int64_t(rows[a] + 1) * row > blob_valid) partial.push_back(a);
  if (int64_t(rows.size()) < kp || !partial.empty()) {  // gather the unverified rows back to back
    plan->check_src_h.assign(rows.size(), 0);
    for (size_t a = 0; a < rows.size(); ++a) plan->check_src_h[a] = int64_t(rows[a]) * row;
    HIP_TRY(plan->check_src.ensure(rows.size() * 8));
    HIP_TRY(plan->check_rows.ensure(rows.size() * size_t(row)));
    HIP_TRY(plan->ctx->upload(plan->check_src.p, plan->check_src_h.data(), rows.size() * 8, st));
    const int full = int(rows.size() - partial.size());  // partial rows are the last ones
    if (full > 0)  // row a of the gather buffer at a * row
      HIP_TRY(rs2k_launch_row_gather(src, plan->check_src.as<int64_t>(),
                                     plan->check_rows.as<uint8_t>(), row, full, st));
    for (size_t a : partial) {
      uint8_t* dst = plan->check_rows.as<uint8_t>() + a * row;
      HIP_TRY(hipMemsetAsync(dst, 0, size_t(row), st));
      const int64_t have = std::max<int64_t>(0, blob_valid - int64_t(rows[a]) * row);
      if (have > 0)
        HIP_TRY(hipMemcpyAsync(dst, src + int64_t(rows[a]) * row, size_t(have),
                               hipMemcpyDeviceToDevice, st));
    }
    src = plan->check_rows.as<uint8_t>();
  }
  HIP_TRY(plan->check_roots.ensure(rows.size() * 32));
  // (st nullptr is the HIP null stream here; at the ABI NULL would mean the verifier's own
  // stream, unordered with the decode that wrote `blob`)
  RS2_TRY(rs2_verifier_roots_device_async(plan->check_v, uint32_t(rows.size()), src,
                                          plan->check_roots.p,
                                          st ? static_cast<void*>(st) : RS2_STREAM_LEGACY));
  std::vector<uint8_t> roots(rows.size() * 32);
  HIP_TRY(hipMemcpyAsync(roots.data(), plan->check_roots.p, roots.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (size_t a = 0; a < rows.size(); ++a)
    if (std::memcmp(roots.data() + 32 * a, hashes + 64 * size_t(rows[a]), 32) != 0)
      return fail(RS2_E_VERIFICATION, "primary sliver hash mismatch");
  return RS2_OK;
}

// Strict consistency check (config.rs:164-172): the metadata of the decoded blob (blob_len bytes
// on the device), re-derived on the device, must give the same blob id.
int strict_check(rs2_plan* plan, const uint8_t* blob_id, const uint8_t* blob, hipStream_t st) {
  RS2_TRY(encode_metadata(plan, blob, plan->pairs.as<uint8_t>(), plan->blob_id.as<uint8_t>(), st));
  uint8_t bid[32];
  HIP_TRY(hipMemcpyAsync(bid, plan->blob_id.p, 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (std::memcmp(bid, blob_id, 32) != 0) return fail(RS2_E_VERIFICATION, "blob id mismatch");
  return RS2_OK;
}

// The consistency check of a blob decoded on the device (`blob_valid` bytes of it written).
// Default, config.rs:621-640: with primary slivers, every systematic index the decoder pulled
// from the input counts as already verified (the caller verified each sliver on receipt); with
// secondary slivers none does.
int check_decoded(rs2_plan* plan, int axis, const uint16_t* sliver_idx, uint32_t pulled,
                  const uint8_t* hashes, const uint8_t* blob_id, int check, const uint8_t* blob,
                  int64_t blob_valid, hipStream_t st) {
  if (check == RS2_CHECK_STRICT) return strict_check(plan, blob_id, blob, st);
  if (check != RS2_CHECK_DEFAULT) return RS2_OK;
  std::vector<uint8_t> verified(plan->kp, 0);
  if (axis == RS2_AXIS_PRIMARY)
    for (uint32_t i = 0; i < pulled; ++i)
      if (sliver_idx[i] < plan->kp) verified[sliver_idx[i]] = 1;
  return default_check(plan, verified, hashes, blob, blob_valid, st);
}

int blob_to_host(rs2_plan* plan, uint8_t* blob_out) {
  if (plan->blob_len) {
    RS2_TRY(stage_d2h(plan->ctx, *plan->stage,
                      {{blob_out, plan->dev_blob.as<uint8_t>(), size_t(plan->blob_len)}},
                      plan->stream));
  }
  HIP_TRY(hipStreamSynchronize(plan->stream));
  return RS2_OK;
}

}  // namespace

extern "C" {

int rs2_decode_blob(rs2_plan* plan, int axis, uint32_t count, const uint16_t* sliver_idx,
                    const uint8_t* const* slivers, const uint64_t* sliver_len,
                    const uint16_t* sliver_symbol_size, uint8_t* blob_out) {
  if (!plan || (!blob_out && plan->blob_len)) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  RingGuard ring(plan);
  RS2_TRY(decode_host(plan, axis, count, sliver_idx, slivers, sliver_len, sliver_symbol_size,
                      nullptr));
  return blob_to_host(plan, blob_out);
}

int rs2_decode_and_verify(rs2_plan* plan, int axis, uint32_t count, const uint16_t* sliver_idx,
                          const uint8_t* const* slivers, const uint64_t* sliver_len,
                          const uint16_t* sliver_symbol_size, const uint8_t* hashes,
                          const uint8_t* blob_id, int consistency_check, uint8_t* blob_out) {
  if (!plan || (!blob_out && plan->blob_len)) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  if (!hashes || !blob_id) return fail(RS2_E_INVALID_ARGUMENT, "null metadata");
  RS2_TRY(check_value(consistency_check));
  RingGuard ring(plan);
  uint32_t pulled = 0;
  RS2_TRY(decode_host(plan, axis, count, sliver_idx, slivers, sliver_len, sliver_symbol_size,
                      &pulled));
  RS2_TRY(check_decoded(plan, axis, sliver_idx, pulled, hashes, blob_id, consistency_check,
                        plan->dev_blob.as<uint8_t>(), int64_t(plan->kp) * plan->ks * plan->s,
                        plan->stream));
  return blob_to_host(plan, blob_out);
}

int rs2_decode_and_verify_device(rs2_plan* plan, int axis, uint32_t count,
                                 const uint16_t* sliver_idx, const void* d_slivers_base,
                                 const uint64_t* sliver_off, const uint8_t* hashes,
                                 const uint8_t* blob_id, int consistency_check, void* d_blob_out,
                                 void* stream) {
  if (!plan || !sliver_idx || !sliver_off || !d_slivers_base || !d_blob_out)
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  if (!hashes || !blob_id) return fail(RS2_E_INVALID_ARGUMENT, "null metadata");
  RS2_TRY(check_axis(axis));
  RS2_TRY(check_value(consistency_check));
  RS2_TRY(check_decode_ptrs(count, d_slivers_base, sliver_off, d_blob_out));
  HIP_TRY(hipSetDevice(plan->ctx->device));
  std::vector<std::pair<uint16_t, uint32_t>> chosen;
  uint32_t pulled = 0;
  RS2_TRY(select_slivers(plan, axis, count, sliver_idx, nullptr, nullptr, chosen, &pulled));
  hipStream_t st = pick_stream(plan, stream);
  uint8_t* out = reinterpret_cast<uint8_t*>(d_blob_out);
  RS2_TRY(decode_device(plan, axis, chosen, reinterpret_cast<const uint8_t*>(d_slivers_base),
                        sliver_off, out, st, plan->blob_len));
  RS2_TRY(check_decoded(plan, axis, sliver_idx, pulled, hashes, blob_id, consistency_check, out,
                        int64_t(plan->blob_len), st));
  HIP_TRY(hipStreamSynchronize(st));
  return RS2_OK;
}

int rs2_encode_1d(uint16_t k, uint16_t n_shards, uint16_t symbol_size, uint32_t batch,
                  const uint8_t* data, uint8_t* out_all) {
  if (!data || !out_all) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  if (symbol_size == 0 || symbol_size % 2)
    return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "symbol_size must be a multiple of the required alignment");
  if (n_shards < k || k == 0)
    return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "n_shards must be at least n_source_symbols");
  Context* ctx = nullptr;
  RS2_TRY(get_context(&ctx));
  const int64_t s = symbol_size, K = k, N = n_shards;
  const size_t in_bytes = size_t(batch) * K * s, out_bytes = size_t(batch) * N * s;
  for (uint32_t b = 0; b < batch; ++b) std::memcpy(out_all + b * N * s, data + b * K * s, K * s);
  if (N == K || batch == 0) return RS2_OK;
  DevBuf din, dout;
  HIP_TRY(din.ensure(in_bytes));
  HIP_TRY(dout.ensure(out_bytes));
  hipStream_t st = ctx->util_stream;
  HIP_TRY(hipMemcpyAsync(din.p, data, in_bytes, hipMemcpyHostToDevice, st));
  PlannedJob pj;
  JobMem mem;
  RS2_TRY(plan_encode(uint32_t(K), uint32_t(N - K), int(s), din.as<uint8_t>(), K * s,
                      [&](uint32_t i) { return int64_t(i) * s; }, dout.as<uint8_t>(), N * s,
                      [&](uint32_t j) { return (K + int64_t(j)) * s; }, INT64_MAX, pj));
  RS2_TRY(bind_job(ctx, pj, mem, st));
  HIP_TRY(launch_job(pj, int(batch), st));
  HIP_TRY(hipStreamSynchronize(st));
  for (uint32_t b = 0; b < batch; ++b)
    HIP_TRY(hipMemcpy(out_all + b * N * s + K * s, dout.as<uint8_t>() + b * N * s + K * s,
                      (N - K) * s, hipMemcpyDeviceToHost));
  return RS2_OK;
}

int rs2_decode_1d(uint16_t k, uint16_t n_shards, uint16_t symbol_size, uint32_t count,
                  const uint16_t* idx, const uint8_t* const* symbols, uint8_t* out_source) {
  if (!out_source || (count && (!idx || !symbols))) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  if (symbol_size == 0 || symbol_size % 2 || n_shards <= k || k == 0)
    return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "incompatible parameters");
  Context* ctx = nullptr;
  RS2_TRY(get_context(&ctx));
  const int64_t s = symbol_size, K = k, N = n_shards;
  std::vector<int64_t> present(N, -1);
  std::vector<uint32_t> order;
  for (uint32_t i = 0; i < count; ++i) {
    if (idx[i] >= N) continue;  // invalid indices are ignored by the crate
    if (present[idx[i]] >= 0) continue;
    present[idx[i]] = int64_t(order.size()) * s;
    order.push_back(i);
  }
  if (order.size() < size_t(K)) return fail(RS2_E_NOT_ENOUGH_SHARDS, "not enough shards");
  // any K shards determine the codeword; use the first K distinct ones
  for (size_t i = size_t(K); i < order.size(); ++i) present[idx[order[i]]] = -1;
  order.resize(size_t(K));
  bool all_src = true;
  for (int64_t i = 0; i < K; ++i) all_src &= present[i] >= 0;
  if (all_src) {
    for (int64_t i = 0; i < K; ++i) {
      const uint32_t src = order[size_t(present[i] / s)];
      std::memcpy(out_source + i * s, symbols[src], s);
    }
    return RS2_OK;
  }
  Dec1DLease lease(ctx, int(K), int(N), int(s));
  HIP_TRY(lease.get());
  Dec1D& D = *lease.d;
  DevBuf& din = D.din;
  DevBuf& dout = D.dout;
  HIP_TRY(din.ensure(order.size() * s));
  HIP_TRY(dout.ensure(K * s));
  hipStream_t st = D.st;
  // the symbols gathered into pinned staging: one DMA instead of K pageable copies
  HIP_TRY(D.hin.ensure(order.size() * s));
  HIP_TRY(D.hout.ensure(size_t(K) * s));
  for (size_t i = 0; i < order.size(); ++i)
    std::memcpy(static_cast<uint8_t*>(D.hin.p) + i * s, symbols[order[i]], s);
  HIP_TRY(hipMemcpyAsync(din.p, D.hin.p, order.size() * s, hipMemcpyHostToDevice, st));
  DecodeSpec sp;
  sp.K = uint32_t(K);
  sp.R = uint32_t(N - K);
  sp.symbol_size = int(s);
  sp.present = present;
  sp.src_base = din.as<uint8_t>();
  sp.src_ls = 0;
  sp.dst_base = dout.as<uint8_t>();
  sp.dst_ls = 0;
  sp.dst.resize(K);
  for (int64_t i = 0; i < K; ++i) sp.dst[i] = i * s;
  RS2_TRY(plan_decode(sp, D.pj));
  RS2_TRY(bind_decode(ctx, D.pj, D.mem, st));
  HIP_TRY(launch_job(D.pj, 1, st));
  HIP_TRY(hipMemcpyAsync(D.hout.p, dout.p, size_t(K) * s, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint8_t* dec = static_cast<const uint8_t*>(D.hout.p);
  for (int64_t i = 0; i < K; ++i) {
    if (present[i] >= 0)
      std::memcpy(out_source + i * s, symbols[order[size_t(present[i] / s)]], s);
    else
      std::memcpy(out_source + i * s, dec + i * s, s);
  }
  return RS2_OK;
}

// ---- sliver verification, Merkle roots, blob ids: all hashing on the device ----------------

int rs2_verifier_create(uint16_t n_shards, uint16_t symbol_size, int axis, rs2_verifier** out) {
  if (!out) return fail(RS2_E_INVALID_ARGUMENT, "null verifier pointer");
  *out = nullptr;
  RS2_TRY(check_axis(axis));
  if (symbol_size == 0 || symbol_size % 2)
    return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "symbol_size must be a multiple of the required alignment");
  uint16_t kp, ks;
  RS2_TRY(rs2_source_symbols_for_n_shards(n_shards, &kp, &ks));
  if (n_shards > kMaxShards) return fail(RS2_E_UNSUPPORTED, "n_shards above 65535");
  Context* ctx = nullptr;
  RS2_TRY(get_context(&ctx));
  auto v = std::make_unique<rs2_verifier>();
  v->ctx = ctx;
  v->n = n_shards;
  v->k = axis == RS2_AXIS_PRIMARY ? ks : kp;  // a primary sliver expands with the secondary code
  v->s = symbol_size;
  v->axis = axis;
  HIP_TRY(hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking));
  *out = v.release();
  return RS2_OK;
}

void rs2_verifier_destroy(rs2_verifier* v) {
  if (!v) return;
  (void)hipSetDevice(v->ctx->device);
  if (v->stream) (void)hipStreamSynchronize(v->stream);
  (void)v->done.sync();  // work queued on a caller's stream
  const Quiesced quiesced;
  delete v;
}

}  // extern "C"

namespace {
// A pooled verifier for one host-buffer call (Context::verifier_pool); returned on scope exit
// with its stream drained (every host-buffer call synchronizes before returning).
struct VerifierLease {
  Context* ctx = nullptr;
  rs2_verifier* v = nullptr;
  VerifierLease() = default;
  VerifierLease(const VerifierLease&) = delete;
  VerifierLease& operator=(const VerifierLease&) = delete;
  int get(uint16_t n_shards, uint16_t symbol_size, int axis) {
    RS2_TRY(get_context(&ctx));
    {
      std::lock_guard<std::mutex> lk(ctx->pool_mu);
      auto& free_ = ctx->verifier_pool[std::make_tuple(int(n_shards), int(symbol_size), axis)];
      if (!free_.empty()) {
        v = free_.back();
        free_.pop_back();
        return RS2_OK;
      }
    }
    return rs2_verifier_create(n_shards, symbol_size, axis, &v);
  }
  ~VerifierLease() {
    if (!v) return;
    // drained before it goes back: an error return may leave the h_in -> input copy queued on
    // its stream, and the next holder rewrites h_in / grows it (PinnedBuf::ensure frees it)
    (void)hipStreamSynchronize(v->stream);
    (void)v->done.sync();
    {
      std::lock_guard<std::mutex> lk(ctx->pool_mu);
      auto& free_ = ctx->verifier_pool[std::make_tuple(int(v->n), int(v->s), v->axis)];
      if (free_.size() < Context::kPoolKeep) {
        free_.push_back(v);
        return;
      }
    }
    rs2_verifier_destroy(v);
  }
};

// path length and node count of a MerkleTree over n leaves (merkle.rs path_length / n_nodes)
int merkle_path_len(uint64_t n) {
  int l = 0;
  while (n > 1) {
    n = (n + 1) / 2;
    ++l;
  }
  return l;
}
uint64_t merkle_n_nodes(uint64_t n) {
  uint64_t tot = 0;
  while (n > 1) {
    n += n & 1;
    tot += n;
    n /= 2;
  }
  return tot + n;
}

// The repair symbols of `count` back-to-back slivers at din (n > k), on st: sliver i's n - k
// symbols at rep + i * (n - k) * s.
int verifier_expand(rs2_verifier* v, const uint8_t* din, uint8_t* rep, int64_t count,
                    hipStream_t st) {
  const int64_t n = v->n, K = v->k, s = v->s;
  RS2_TRY(plan_encode(uint32_t(K), uint32_t(n - K), int(s), din, K * s,
                      [&](uint32_t i) { return int64_t(i) * s; }, rep, (n - K) * s,
                      [&](uint32_t j) { return int64_t(j) * s; }, INT64_MAX, v->job));
  RS2_TRY(bind_job(v->ctx, v->job, v->mem, st));
  HIP_TRY(launch_job(v->job, int(count), st));
  return RS2_OK;
}

// The n leaf hashes (v->leaves) of `count` back-to-back slivers, on st, without an expanded
// copy: each sliver's n - k repair symbols on the orthogonal axis go to a compact
// [count][n - k][s] buffer (v->repair) and the leaf kernel reads its systematic symbols in place
// (rs2k_launch_leaf_hash mode 4); recovery symbols gather from the same two places
// (proof_gather_kernel).
int verifier_leaves(rs2_verifier* v, uint32_t count, const uint8_t* din, hipStream_t st) {
  const int64_t n = v->n, K = v->k, s = v->s;
  // a previous call on another stream still owns the scratch buffers: order after it, so the
  // done event recorded at the end of this call also covers that one
  HIP_TRY(v->done.wait_on(st));
  HIP_TRY(v->leaves.ensure(size_t(count) * n * 32));
  uint8_t* rep = nullptr;
  if (n > K) {
    HIP_TRY(v->repair.ensure(size_t(count) * (n - K) * s));
    rep = v->repair.as<uint8_t>();
    RS2_TRY(verifier_expand(v, din, rep, count, st));
  }
  SymbolMap map{din, rep, nullptr, int(n), int(count), int(K), int(s)};
  HIP_TRY(rs2k_launch_leaf_hash(map, 4, int64_t(count) * n, 1, v->leaves.as<uint8_t>(), st));
  return RS2_OK;
}

// the verifier's last work on st (any caller stream): rs2_verifier_destroy waits for it
int verifier_mark_done(rs2_verifier* v, hipStream_t st) {
  HIP_TRY(v->done.record(st));
  return RS2_OK;
}

// the hashing scratch for `count` slivers at once, so that no run of a window regrows it in flight
int verifier_reserve(rs2_verifier* v, size_t count) {
  HIP_TRY(v->leaves.ensure(count * size_t(v->n) * 32));
  HIP_TRY(v->repair.ensure(count * size_t(v->n - v->k) * size_t(v->s)));
  if (const size_t sb = tree_scratch_bytes(int64_t(count), v->n)) HIP_TRY(v->tree_scratch.ensure(sb));
  return RS2_OK;
}

// Merkle roots of `count` back-to-back slivers into d_roots (32 B each), on st.
int verifier_roots(rs2_verifier* v, uint32_t count, const uint8_t* d_slivers, uint8_t* d_roots,
                   hipStream_t st) {
  RS2_TRY(verifier_leaves(v, count, d_slivers, st));
  uint8_t* scratch = nullptr;
  if (const size_t sb = tree_scratch_bytes(count, v->n)) {
    HIP_TRY(v->tree_scratch.ensure(sb));
    scratch = v->tree_scratch.as<uint8_t>();
  }
  HIP_TRY(rs2k_launch_merkle_trees(v->leaves.as<uint8_t>(), int(v->n), int(count), 0,
                                   int64_t(v->n) * 32, 32, 0, 0, d_roots, 32, st, nullptr, 0, 1, 0,
                                   0, scratch));
  return RS2_OK;
}

// ---------------------------------------------------------------------------------------------
// sliver recovery: many slivers of the verifier's axis, a received symbol set per sliver
// ---------------------------------------------------------------------------------------------
std::atomic<uint64_t> g_recover_launches{0}, g_recover_batched{0}, g_recover_single{0};

// One validated sliver of a recovery call: its slot in the call, its first symbol in the call's
// symbol buffer and the symbols it is recovered from (select_recovery_symbols).
struct RecoverItem {
  uint32_t slot = 0;
  size_t first = 0;
  std::vector<std::pair<uint16_t, uint32_t>> chosen;
};

// The per-sliver rules of a recovery call for every sliver (status_out as for
// rs2_decode_batch_device_async): the accepted slivers in `items`, in slot order.
int validate_recovery(const rs2_verifier* v, uint32_t n_slivers, const uint32_t* counts,
                      const uint16_t* symbol_idx, int* status_out, std::vector<RecoverItem>& items) {
  items.clear();
  items.reserve(n_slivers);
  size_t first = 0;
  for (uint32_t i = 0; i < n_slivers; first += counts[i], ++i) {
    RecoverItem it;
    it.slot = i;
    it.first = first;
    bool ok;
    RS2_TRY(slot_outcome(select_recovery_symbols(v->k, v->n, counts[i], symbol_idx + first, it.chosen),
                         status_out, i, &ok));
    if (ok) items.push_back(std::move(it));
  }
  return RS2_OK;
}

// Recover validated slivers (slot order) on st: windows of at most a chunk's jobs are planned on
// the host pool; a window's eligible slivers leave in chunks (one launch each, one line per
// job), the others through the per-pattern decode; then the window's roots and verdicts.
// Slots of the call that are not in `items` were refused: their verdict is RS2_SLIVER_SKIPPED.
int recover_items(rs2_verifier* v, uint32_t n_slivers, const std::vector<RecoverItem>& items,
                  const uint8_t* d_symbols, const uint8_t* expected_roots, uint8_t* d_out,
                  uint8_t* d_roots, int32_t* d_verdict, hipStream_t st) {
  Context* ctx = v->ctx;
  const int64_t s = v->s, K = v->k;
  const size_t sliver_len = size_t(K) * size_t(s);
  // a previous call on another stream still owns the scratch buffers (verifier_mark_done)
  HIP_TRY(v->done.wait_on(st));
  const bool want_roots = d_roots || expected_roots;
  const BatchRun run{ctx, v->rbatch, v->rbatch_slot, 1, &v->prof, "rec_plan_host",
                     g_recover_launches, g_recover_batched, g_recover_single};
  size_t next_item = 0;
  for (uint32_t w0 = 0; w0 < n_slivers; w0 += uint32_t(kBatchChunkJobs)) {
    const uint32_t w1 = uint32_t(std::min<size_t>(n_slivers, size_t(w0) + kBatchChunkJobs));
    const size_t i0 = next_item;
    while (next_item < items.size() && items[next_item].slot < w1) ++next_item;
    const size_t cnt = next_item - i0;
    std::vector<DecodeSpec> specs(cnt);
    RS2_TRY(run_batch_window(
        run, cnt, st,
        [&](size_t i, BatchBlob& bb) {
          const RecoverItem& it = items[i0 + i];
          DecodeSpec& sp = specs[i];
          sliver_recover_spec(uint32_t(K), v->n, int(s), it.chosen, d_symbols + it.first * s,
                              d_out + size_t(it.slot) * sliver_len, decode_may_fuse(), sp);
          uint32_t originals = 0;
          for (uint32_t q = 0; q < sp.K; ++q) originals += sp.present[q] >= 0;
          if (originals < sp.K) plan_batch_spec(sp, originals, bb);
        },
        [&](size_t i) {
          return run_decode(ctx, v->rdec, v->rdec_slot, specs[i], {}, decode_may_fuse(), 1,
                            &v->prof, st);
        }));
    if (!want_roots) continue;
    mark(&v->prof, "", st);
    // roots of the window's recovered slivers, in runs of neighbouring slots (a refused sliver
    // leaves a gap: its output was not written and its root slot is not either)
    uint8_t* roots = d_roots ? d_roots + size_t(w0) * 32 : nullptr;  // of slot w0
    if (!roots) {
      HIP_TRY(v->window_roots.ensure(kBatchChunkJobs * 32));
      roots = v->window_roots.as<uint8_t>();
    }
    // the hashing scratch once, for the longest run: no run regrows it in flight
    if (cnt) RS2_TRY(verifier_reserve(v, cnt));
    RS2_TRY(for_each_run(
        i0, next_item, [&](size_t i) { return items[i].slot; },
        [&](size_t a, size_t b) {
          const uint32_t slot = items[a].slot;
          return verifier_roots(v, uint32_t(b - a), d_out + size_t(slot) * sliver_len,
                                roots + size_t(slot - w0) * 32, st);
        }));
    mark(&v->prof, "rec_roots", st);
    if (!expected_roots) continue;
    // expected roots and skip mask of the window through one upload slot
    const uint32_t wn = w1 - w0;
    const size_t mask_at = size_t(wn) * 32;
    std::vector<uint8_t> up(mask_at + wn, 1);
    std::memcpy(up.data(), expected_roots + size_t(w0) * 32, mask_at);
    for (size_t i = 0; i < cnt; ++i) up[mask_at + (items[i0 + i].slot - w0)] = 0;
    HIP_TRY(v->verdict_in.ensure(kBatchChunkJobs * 33));
    RS2_TRY(upload_pieces(ctx, v->verdict_in.p, up.data(), up.size(), st));
    HIP_TRY(rs2k_launch_sliver_verdict(roots, v->verdict_in.as<uint8_t>(),
                                       v->verdict_in.as<uint8_t>() + mask_at, int(wn),
                                       d_verdict + w0, st));
    mark(&v->prof, "rec_verdict", st);
  }
  return RS2_OK;
}

// ---------------------------------------------------------------------------------------------
// verified decode batches: many blobs, each decoded from its own slivers and checked against its
// own metadata, a verdict per blob in device memory
// ---------------------------------------------------------------------------------------------
constexpr uint64_t kVerifyBatchBudget = uint64_t(256) << 20;
std::atomic<uint64_t> g_vb_budget{kVerifyBatchBudget};
std::atomic<uint64_t> g_vb_windows{0}, g_vb_blobs{0}, g_vb_rows{0}, g_vb_encoded{0};

// Decode and check validated blobs (slot order; it.blob = the slot) of a call of n_slots slots on
// st.  Slot b's metadata is at d_hashes + b*64n / d_ids + b*32, its verdict at d_verdict + b;
// accepted blobs lie out_stride apart.  Slots that are not in `items` were refused:
// RS2_BLOB_SKIPPED.  The slots are cut into windows (verify_windows: at most a decode chunk's
// blobs, check scratch within the budget); per window the decodes, then the checks -- Default:
// the unverified rows of every blob gathered back to back and hashed by one verifier_roots;
// Strict: the blobs re-encoded in runs of neighbouring accepted slots -- then one verdict launch.
// Every scratch buffer is sized for the largest window before the first one runs, so nothing is
// re-allocated with work in flight and the call never waits for the device.
int verify_batch_items(rs2_plan* p, int axis, uint32_t n_slots, const std::vector<BatchItem>& items,
                       const uint8_t* base, const uint8_t* d_hashes, const uint8_t* d_ids,
                       int check, int32_t* d_verdict, uint64_t out_stride, hipStream_t st) {
  Context* ctx = p->ctx;
  const int64_t n = p->n, kp = p->kp, ks = p->ks, s = p->s;
  const int64_t row = ks * s, pl = primary_len(p), sl = secondary_len(p);
  const int64_t both_b = (n - kp) * (n - ks) * s, leaves_b = n * n * 32;
  const bool dflt = check == RS2_CHECK_DEFAULT, strict = check == RS2_CHECK_STRICT;
  // per slot: the rows to hash (Default) and the check scratch
  std::vector<std::vector<VerifyRow>> rows(dflt ? items.size() : 0);
  std::vector<uint64_t> need(n_slots, 0);
  const uint64_t row_need = uint64_t(row) + uint64_t(n) * 32 + uint64_t(n - ks) * s;
  const uint64_t strict_need = uint64_t(n) * (pl + sl) + uint64_t(both_b) + uint64_t(leaves_b);
  for (size_t i = 0; i < items.size(); ++i) {
    const BatchItem& it = items[i];
    if (dflt) {
      verify_rows(uint32_t(kp), uint32_t(ks), uint32_t(s), axis, it.idx, it.pulled, it.len, rows[i]);
      need[it.blob] = rows[i].size() * row_need;
    } else if (strict) {
      need[it.blob] = strict_need;
    }
  }
  std::vector<uint32_t> ends;
  verify_windows(need, g_vb_budget.load(std::memory_order_relaxed), kBatchChunkJobs, ends);
  // the largest window: accepted blobs and rows
  size_t max_cnt = 0, max_rows = 0;
  {
    size_t i = 0;
    for (uint32_t w1 : ends) {
      size_t cnt = 0, nr = 0;
      for (; i < items.size() && items[i].blob < w1; ++i, ++cnt)
        if (dflt) nr += rows[i].size();
      max_cnt = std::max(max_cnt, cnt);
      max_rows = std::max(max_rows, nr);
    }
  }
  // the previous call's work (possibly on another stream) still owns the scratch
  HIP_TRY(p->vb_done.wait_on(st));
  HIP_TRY(p->vb_slot_tab.ensure(kBatchChunkJobs * sizeof(CheckSlot)));
  rs2_verifier* v = nullptr;
  if (dflt && max_rows) {
    if (!p->check_v) RS2_TRY(rs2_verifier_create(p->n, p->s, RS2_AXIS_PRIMARY, &p->check_v));
    v = p->check_v;
    HIP_TRY(p->vb_row_tab.ensure(max_rows * sizeof(CheckRow)));
    HIP_TRY(p->vb_rows.ensure(max_rows * size_t(row)));
    HIP_TRY(p->vb_roots.ensure(max_rows * 32));
    RS2_TRY(verifier_reserve(v, max_rows));
  }
  if (strict && max_cnt) {
    HIP_TRY(p->vb_primary.ensure(max_cnt * size_t(n * pl)));
    HIP_TRY(p->vb_secondary.ensure(max_cnt * size_t(n * sl)));
    HIP_TRY(p->vb_hashes.ensure(max_cnt * size_t(n) * 64));
    HIP_TRY(p->vb_ids.ensure(kBatchChunkJobs * 32));
    HIP_TRY(p->batch_both.ensure(max_cnt * size_t(both_b)));
    HIP_TRY(p->batch_leaves.ensure(max_cnt * size_t(leaves_b)));
    if (const size_t sb = tree_scratch_bytes(2 * n, n)) HIP_TRY(p->tree_scratch.ensure(sb));
    // the call's blob lengths by slot, once (refused slots: 0, never read)
    std::vector<uint64_t> lens(n_slots, 0);
    for (const BatchItem& it : items) lens[it.blob] = it.len;
    HIP_TRY(p->vb_lens.ensure(lens.size() * 8));
    RS2_TRY(upload_pieces(ctx, p->vb_lens.p, lens.data(), lens.size() * 8, st));
  }
  size_t next_item = 0;
  uint32_t w0 = 0;
  for (uint32_t w1 : ends) {
    const uint32_t wn = w1 - w0;
    const size_t i0 = next_item;
    while (next_item < items.size() && items[next_item].blob < w1) ++next_item;
    const size_t cnt = next_item - i0;
    // 1. the window's decodes
    if (cnt) {
      const std::vector<BatchItem> part(items.begin() + i0, items.begin() + next_item);
      RS2_TRY(decode_batch_items(p, axis, part, base, st));
    }
    // 2. its checks
    std::vector<CheckSlot> slots(wn, CheckSlot{0, kCheckSkipped});
    size_t n_rows = 0;
    if (dflt) {
      std::vector<CheckRow> tab;
      for (size_t i = i0; i < next_item; ++i) {
        const BatchItem& it = items[i];
        slots[it.blob - w0] = CheckSlot{uint32_t(tab.size()), uint32_t(rows[i].size())};
        for (const VerifyRow& r : rows[i])
          tab.push_back(CheckRow{it.out + int64_t(r.row) * row, r.valid, r.row});
      }
      n_rows = tab.size();
      if (n_rows) {
        mark(p, "", st);
        RS2_TRY(upload_pieces(ctx, p->vb_row_tab.p, tab.data(), n_rows * sizeof(CheckRow), st));
        HIP_TRY(rs2k_launch_check_rows_gather(p->vb_row_tab.as<CheckRow>(), int64_t(n_rows), row,
                                              p->vb_rows.as<uint8_t>(), st));
        mark(p, "ver_batch_rows", st);
        RS2_TRY(verifier_roots(v, uint32_t(n_rows), p->vb_rows.as<uint8_t>(),
                               p->vb_roots.as<uint8_t>(), st));
        mark(p, "ver_batch_roots", st);
      }
    } else {
      for (size_t i = i0; i < next_item; ++i) slots[items[i].blob - w0] = CheckSlot{0, 0};
    }
    if (strict && cnt) {
      mark(p, "", st);
      const bool prof_on = p->prof.on;
      p->prof.on = false;  // one stage for the window's encodes, not encode_batch_device's own
      // runs of neighbouring accepted slots: a refused blob's slot is never read
      const int rc = for_each_run(
          i0, next_item, [&](size_t i) { return items[i].blob; },
          [&](size_t a, size_t b) {
            const uint32_t slot = items[a].blob;
            std::vector<uint64_t> lens(b - a);
            for (size_t i = a; i < b; ++i) lens[i - a] = items[i].len;
            return encode_batch_device(
                p, uint32_t(b - a), items[a].out, int64_t(out_stride), lens.data(),
                p->vb_primary.as<uint8_t>(), n * pl, p->vb_secondary.as<uint8_t>(), n * sl,
                p->vb_hashes.as<uint8_t>(), p->vb_ids.as<uint8_t>() + size_t(slot - w0) * 32, st,
                p->vb_lens.as<uint64_t>() + slot);
          });
      p->prof.on = prof_on;
      RS2_TRY(rc);
      mark(p, "ver_batch_encode", st);
      g_vb_encoded.fetch_add(cnt, std::memory_order_relaxed);
    }
    // 3. its verdicts
    mark(p, "", st);
    RS2_TRY(upload_pieces(ctx, p->vb_slot_tab.p, slots.data(), wn * sizeof(CheckSlot), st));
    if (strict)
      HIP_TRY(rs2k_launch_blob_verdict(p->vb_slot_tab.as<CheckSlot>(), int(wn), nullptr,
                                       p->vb_ids.as<uint8_t>(), d_ids + size_t(w0) * 32, 32, 1,
                                       d_verdict + w0, st));
    else
      HIP_TRY(rs2k_launch_blob_verdict(p->vb_slot_tab.as<CheckSlot>(), int(wn),
                                       p->vb_row_tab.as<CheckRow>(), p->vb_roots.as<uint8_t>(),
                                       dflt ? d_hashes + size_t(w0) * 64 * size_t(n) : nullptr,
                                       64 * n, 0, d_verdict + w0, st));
    mark(p, "ver_batch_verdict", st);
    g_vb_windows.fetch_add(1, std::memory_order_relaxed);
    if (dflt || strict) g_vb_blobs.fetch_add(cnt, std::memory_order_relaxed);
    g_vb_rows.fetch_add(n_rows, std::memory_order_relaxed);
    w0 = w1;
  }
  if (v) RS2_TRY(verifier_mark_done(v, st));
  HIP_TRY(p->vb_done.record(st));
  return RS2_OK;
}

// The argument rules the two forms of the verified batch share.
int check_verify_batch_args(int check, const void* hashes, const void* blob_ids,
                            const void* verdict) {
  RS2_TRY(check_value(check));
  if (!verdict) return fail(RS2_E_INVALID_ARGUMENT, "null verdicts");
  if (check == RS2_CHECK_DEFAULT && !hashes) return fail(RS2_E_INVALID_ARGUMENT, "null hashes");
  if (check == RS2_CHECK_STRICT && !blob_ids) return fail(RS2_E_INVALID_ARGUMENT, "null blob ids");
  return RS2_OK;
}

// The host-buffer batch decode, plain (check == kNoCheck: rs2_decode_batch) or verified
// (rs2_decode_and_verify_batch).
constexpr int kNoCheck = -1;
int decode_batch_host(rs2_plan* plan, int axis, uint32_t n_blobs, const uint64_t* blob_lens,
                      const uint32_t* counts, const uint16_t* sliver_idx,
                      const uint8_t* const* slivers, const uint64_t* sliver_len,
                      const uint16_t* sliver_symbol_size, const uint8_t* hashes,
                      const uint8_t* blob_ids, int check, uint8_t* const* blobs_out,
                      int32_t* verdict_out, int* status_out) {
  if (!plan) return fail(RS2_E_INVALID_ARGUMENT, "null plan");
  RS2_TRY(check_axis(axis));
  const bool verify = check != kNoCheck;
  if (verify) RS2_TRY(check_verify_batch_args(check, hashes, blob_ids, verdict_out));
  bool empty;
  RS2_TRY(batch_count(n_blobs, "blobs in a batch", counts && blobs_out, &empty));
  if (empty) return RS2_OK;
  if (std::accumulate(counts, counts + n_blobs, size_t(0)) && (!sliver_idx || !slivers || !sliver_len))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(plan->ctx->device));
  RingGuard ring(plan);
  Context* ctx = plan->ctx;
  hipStream_t st = plan->stream;
  const size_t len = size_t(axis == RS2_AXIS_PRIMARY ? primary_len(plan) : secondary_len(plan));
  const uint32_t K = axis == RS2_AXIS_PRIMARY ? plan->kp : plan->ks;
  const size_t msg = size_t(plan->kp) * plan->ks * plan->s;
  const size_t ostride = (std::max<size_t>(msg, 16) + 255) / 256 * 256;
  const size_t hashes_b = size_t(plan->n) * 64;
  std::vector<BatchItem> items;
  items.reserve(n_blobs);
  size_t first = 0;
  for (uint32_t b = 0; b < n_blobs; first += counts[b], ++b) {
    BatchItem it;
    it.blob = b;
    it.idx = sliver_idx + first;
    auto validate = [&]() -> int {
      RS2_TRY(batch_blob_len(plan, blob_lens, b, &it.len));
      if (it.len && !blobs_out[b]) return fail(RS2_E_INVALID_ARGUMENT, "null output blob");
      RS2_TRY(select_slivers(plan, axis, counts[b], sliver_idx + first, sliver_len + first,
                             sliver_symbol_size ? sliver_symbol_size + first : nullptr, it.chosen,
                             &it.pulled));
      for (const auto& c : it.chosen)
        if (!slivers[first + c.second]) return fail(RS2_E_INVALID_ARGUMENT, "null sliver");
      return RS2_OK;
    };
    bool ok;
    RS2_TRY(slot_outcome(validate(), status_out, b, &ok));
    if (!ok) continue;
    for (auto& c : it.chosen) c.second = uint32_t(first + c.second);  // position in `slivers`
    items.push_back(std::move(it));
  }
  if (verify) std::fill(verdict_out, verdict_out + n_blobs, int32_t(RS2_BLOB_SKIPPED));
  // groups of blobs whose device slivers and outputs stay below a fixed budget
  constexpr size_t kGroupBytes = size_t(512) << 20;
  const size_t per_blob = size_t(K) * len + ostride;
  const size_t group = std::max<size_t>(1, kGroupBytes / per_blob);
  for (size_t g0 = 0; g0 < items.size(); g0 += group) {
    const size_t g1 = std::min(items.size(), g0 + group), nb = g1 - g0;
    HIP_TRY(plan->dbatch_in.ensure(nb * size_t(K) * len));
    HIP_TRY(plan->dbatch_out.ensure(nb * ostride));
    uint8_t* din = plan->dbatch_in.as<uint8_t>();
    uint8_t* dout = plan->dbatch_out.as<uint8_t>();
    std::vector<Seg> segs;
    std::vector<std::vector<uint64_t>> offs(nb);
    std::vector<BatchItem> part(items.begin() + g0, items.begin() + g1);
    // the chosen slivers go to the device back to back: sliver k of the group's blob i at
    // (i * K + k) * len
    for (size_t i = 0; i < nb; ++i) {
      BatchItem& it = part[i];
      offs[i].resize(it.chosen.size());
      for (size_t k = 0; k < it.chosen.size(); ++k) {
        const size_t at = (i * K + k) * len;
        segs.push_back({const_cast<uint8_t*>(slivers[it.chosen[k].second]), din + at, len});
        offs[i][k] = at;
        it.chosen[k].second = uint32_t(k);
      }
      it.off = offs[i].data();
      it.out = dout + i * ostride;
    }
    if (!verify) {
      RS2_TRY(stage_h2d(ctx, *plan->stage, segs, st));
      RS2_TRY(decode_batch_items(plan, axis, part, din, st));
    } else {
      // the group's metadata beside its slivers, by the group's own slots 0 .. nb
      uint8_t *dh = nullptr, *di = nullptr;
      if (check == RS2_CHECK_DEFAULT) {
        HIP_TRY(plan->vb_h_hashes.ensure(nb * hashes_b));
        dh = plan->vb_h_hashes.as<uint8_t>();
      } else if (check == RS2_CHECK_STRICT) {
        HIP_TRY(plan->vb_h_ids.ensure(nb * 32));
        di = plan->vb_h_ids.as<uint8_t>();
      }
      HIP_TRY(plan->vb_h_verdict.ensure(nb * 4));
      for (size_t i = 0; i < nb; ++i) {
        const size_t b = part[i].blob;
        if (dh) segs.push_back({const_cast<uint8_t*>(hashes) + b * hashes_b, dh + i * hashes_b, hashes_b});
        if (di) segs.push_back({const_cast<uint8_t*>(blob_ids) + b * 32, di + i * 32, 32});
        part[i].blob = uint32_t(i);
      }
      RS2_TRY(stage_h2d(ctx, *plan->stage, segs, st));
      RS2_TRY(verify_batch_items(plan, axis, uint32_t(nb), part, din, dh, di, check,
                                 plan->vb_h_verdict.as<int32_t>(), ostride, st));
    }
    segs.clear();
    for (size_t i = 0; i < nb; ++i)
      if (items[g0 + i].len)
        segs.push_back({blobs_out[items[g0 + i].blob], dout + i * ostride, size_t(items[g0 + i].len)});
    std::vector<int32_t> verdicts(verify ? nb : 0);
    if (verify)
      segs.push_back({reinterpret_cast<uint8_t*>(verdicts.data()), plan->vb_h_verdict.as<uint8_t>(), nb * 4});
    if (!segs.empty()) RS2_TRY(stage_d2h(ctx, *plan->stage, segs, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < verdicts.size(); ++i) verdict_out[items[g0 + i].blob] = verdicts[i];
  }
  return RS2_OK;
}

// ---------------------------------------------------------------------------------------------
// recovery symbols in bulk: many source slivers, a list of targets per sliver
// ---------------------------------------------------------------------------------------------
constexpr uint64_t kSymbolsBudget = uint64_t(256) << 20;
std::atomic<uint64_t> g_sym_budget{kSymbolsBudget};
std::atomic<uint64_t> g_sym_windows{0}, g_sym_expanded{0}, g_sym_built{0}, g_sym_cached{0},
    g_sym_requests{0};
// requests of one gather launch: the device copy of the request table never holds more
constexpr uint32_t kRequestChunk = 1u << 20;

// The windows of a planned bulk call (plan_symbol_requests) on st, one after the other: per run
// of slivers to expand, the codec into the window's repair scratch and with BUILD the leaf hashes
// and trees (node arrays into d_nodes, or into scratch when the caller takes none); then the
// window's requests in chunks, table upload and gather.  The scratch is sized by the largest
// window and reused in stream order.  With CACHED d_nodes is only read.
int symbol_request_windows(rs2_verifier* v, const SymbolRequestPlan& plan,
                           const uint32_t* target_counts, int trees, const uint8_t* d_slivers,
                           uint8_t* d_nodes, uint8_t* d_symbols, uint8_t* d_proofs,
                           hipStream_t st) {
  const int64_t n = v->n, K = v->k, s = v->s, nn = int64_t(plan.n_nodes), L = plan.path_len;
  const bool build = trees == RS2_TREES_BUILD;
  // a previous call on another stream still owns the scratch buffers (verifier_leaves)
  HIP_TRY(v->done.wait_on(st));
  size_t widest = 0;
  bool codec = false, runs = false;
  for (const SymbolWindow& w : plan.windows) {
    widest = std::max<size_t>(widest, w.n_slivers);
    codec |= w.needs_codec;
    runs |= !w.runs.empty();
  }
  if (codec) HIP_TRY(v->repair.ensure(widest * size_t(n - K) * s));
  if (build && runs) {
    HIP_TRY(v->leaves.ensure(widest * size_t(n) * 32));
    HIP_TRY(v->roots.ensure(widest * 32));
    if (!d_nodes) HIP_TRY(v->nodes.ensure(widest * size_t(nn) * 32));
  }
  if (plan.total)
    HIP_TRY(v->requests.ensure(size_t(std::min<uint64_t>(plan.total, kRequestChunk)) * 4));
  SymbolLevels lv;
  std::copy(plan.level_base, plan.level_base + kSymbolLevels, lv.base);
  uint64_t expanded = 0, built = 0;
  for (const SymbolWindow& w : plan.windows) {
    const uint8_t* din = d_slivers + int64_t(w.first_sliver) * K * s;
    uint8_t* nodes = d_nodes ? d_nodes + int64_t(w.first_sliver) * nn * 32 : v->nodes.as<uint8_t>();
    for (const auto& run : w.runs) {
      const int64_t first = run.first, cnt = run.second;
      const uint8_t* rin = din + first * K * s;
      uint8_t* rep = nullptr;
      if (n > K) {
        rep = v->repair.as<uint8_t>() + first * (n - K) * s;
        RS2_TRY(verifier_expand(v, rin, rep, cnt, st));
        expanded += uint64_t(cnt);
      }
      if (!build) continue;
      uint8_t* leaves = v->leaves.as<uint8_t>() + first * n * 32;
      SymbolMap map{rin, rep, nullptr, int(n), int(cnt), int(K), int(s)};
      HIP_TRY(rs2k_launch_leaf_hash(map, 4, cnt * n, 1, leaves, st));
      HIP_TRY(rs2k_launch_merkle_trees(leaves, int(n), int(cnt), 0, n * 32, 32, 0, 0,
                                       v->roots.as<uint8_t>() + first * 32, 32, st,
                                       nodes + first * nn * 32, nn * 32));
      built += uint64_t(cnt);
    }
    for (uint32_t c0 = 0; c0 < w.n_requests; c0 += kRequestChunk) {
      const uint32_t cn = std::min(kRequestChunk, w.n_requests - c0);
      const int64_t r0 = int64_t(w.first_request) + c0;
      // through the pinned slot ring: the caller's arrays and the plan's table may go at once
      RS2_TRY(upload_pieces(v->ctx, v->requests.p, plan.table.data() + r0, size_t(cn) * 4, st));
      HIP_TRY(rs2k_launch_symbol_requests(din, v->repair.as<uint8_t>(), int(n), int(K), int(s),
                                          nodes, nn * 32, v->requests.as<uint32_t>(), cn, int(L),
                                          lv, d_symbols + r0 * s, d_proofs + r0 * L * 32, st));
    }
  }
  uint64_t served_trees = 0;
  if (!build)
    for (const SymbolWindow& w : plan.windows)
      for (uint32_t i = 0; i < w.n_slivers; ++i) served_trees += target_counts[w.first_sliver + i] > 0;
  g_sym_windows.fetch_add(plan.windows.size(), std::memory_order_relaxed);
  g_sym_expanded.fetch_add(expanded, std::memory_order_relaxed);
  g_sym_built.fetch_add(built, std::memory_order_relaxed);
  g_sym_cached.fetch_add(served_trees, std::memory_order_relaxed);
  g_sym_requests.fetch_add(plan.total, std::memory_order_relaxed);
  return RS2_OK;
}

// ---------------------------------------------------------------------------------------------
// host-buffer forms: a pooled verifier, its pinned h_in / h_out and its own stream
// ---------------------------------------------------------------------------------------------
// The length rule of the host-buffer forms: `count` slivers of k * s bytes each.
int check_host_slivers(const rs2_verifier* v, uint32_t count, const uint8_t* const* slivers,
                       const uint64_t* sliver_len) {
  const uint64_t len = uint64_t(v->k) * v->s;
  for (uint32_t i = 0; i < count; ++i)
    if (!slivers[i] || sliver_len[i] != len)
      return fail(RS2_E_INCORRECT_DATA_LENGTH, "sliver length does not match the encoder");
  return RS2_OK;
}

// The checked slivers gathered into pinned staging and on to v->input: one DMA, not a pageable
// copy per sliver.  (Apart from the check: a call makes all its checks before it queues work.)
// h_out is sized for the call's out_bytes here, before any work is queued.
int upload_host_slivers(rs2_verifier* v, uint32_t count, const uint8_t* const* slivers,
                        size_t out_bytes) {
  const size_t len = size_t(v->k) * v->s;
  HIP_TRY(v->input.ensure(count * len));
  HIP_TRY(v->h_in.ensure(count * len));
  HIP_TRY(v->h_out.ensure(out_bytes));
  for (uint32_t i = 0; i < count; ++i)
    std::memcpy(static_cast<uint8_t*>(v->h_in.p) + i * len, slivers[i], len);
  HIP_TRY(hipMemcpyAsync(v->input.p, v->h_in.p, count * len, hipMemcpyHostToDevice, v->stream));
  return RS2_OK;
}

// Device ranges back to the host after the work queued on the verifier's stream: one D2H each
// (none for an empty range) into h_out, which the call sized before it queued work, back to back
// in the order given, one synchronize.
using DevRange = std::pair<const void*, size_t>;  // device address, bytes
int download_ranges(rs2_verifier* v, std::initializer_list<DevRange> ranges, const uint8_t** host) {
  uint8_t* ho = static_cast<uint8_t*>(v->h_out.p);
  size_t at = 0;
  for (const DevRange& r : ranges) {
    if (r.second) HIP_TRY(hipMemcpyAsync(ho + at, r.first, r.second, hipMemcpyDeviceToHost, v->stream));
    at += r.second;
  }
  HIP_TRY(hipStreamSynchronize(v->stream));
  *host = ho;
  return RS2_OK;
}

}  // namespace

extern "C" {

int rs2_decode_and_verify_batch_device_async(
    rs2_plan* plan, int axis, uint32_t n_blobs, const uint64_t* blob_lens, const uint32_t* counts,
    const uint16_t* sliver_idx, const void* d_slivers_base, const uint64_t* sliver_off,
    const void* d_hashes, const void* d_blob_ids, int consistency_check, void* d_blobs_out,
    uint64_t out_stride, void* d_verdict, int* status_out, void* stream) {
  if (!plan) return fail(RS2_E_INVALID_ARGUMENT, "null plan");
  RS2_TRY(check_axis(axis));
  RS2_TRY(check_verify_batch_args(consistency_check, d_hashes, d_blob_ids, d_verdict));
  RS2_TRY(check_digest_ptr(d_hashes, "d_hashes"));
  RS2_TRY(check_digest_ptr(d_blob_ids, "d_blob_ids"));
  RS2_TRY(check_digest_ptr(d_verdict, "d_verdict"));
  bool empty;
  RS2_TRY(batch_count(n_blobs, "blobs in a batch",
                      counts && sliver_idx && sliver_off && d_slivers_base && d_blobs_out, &empty));
  if (empty) return RS2_OK;
  RS2_TRY(check_symbol_ptr(d_slivers_base, "d_slivers_base"));
  RS2_TRY(check_symbol_ptr(d_blobs_out, "d_blobs_out"));
  RS2_TRY(check_symbol_step(out_stride, "out_stride"));
  HIP_TRY(hipSetDevice(plan->ctx->device));
  // every blob is validated before anything is enqueued
  std::vector<BatchItem> items;
  RS2_TRY(validate_batch_device(plan, axis, n_blobs, blob_lens, counts, sliver_idx, sliver_off,
                                d_blobs_out, out_stride, status_out, items));
  return verify_batch_items(plan, axis, n_blobs, items,
                            reinterpret_cast<const uint8_t*>(d_slivers_base),
                            reinterpret_cast<const uint8_t*>(d_hashes),
                            reinterpret_cast<const uint8_t*>(d_blob_ids), consistency_check,
                            reinterpret_cast<int32_t*>(d_verdict), out_stride,
                            pick_stream(plan, stream));
}

int rs2_decode_batch(rs2_plan* plan, int axis, uint32_t n_blobs, const uint64_t* blob_lens,
                     const uint32_t* counts, const uint16_t* sliver_idx,
                     const uint8_t* const* slivers, const uint64_t* sliver_len,
                     const uint16_t* sliver_symbol_size, uint8_t* const* blobs_out,
                     int* status_out) {
  return decode_batch_host(plan, axis, n_blobs, blob_lens, counts, sliver_idx, slivers, sliver_len,
                           sliver_symbol_size, nullptr, nullptr, kNoCheck, blobs_out, nullptr,
                           status_out);
}

int rs2_decode_and_verify_batch(rs2_plan* plan, int axis, uint32_t n_blobs,
                                const uint64_t* blob_lens, const uint32_t* counts,
                                const uint16_t* sliver_idx, const uint8_t* const* slivers,
                                const uint64_t* sliver_len, const uint16_t* sliver_symbol_size,
                                const uint8_t* hashes, const uint8_t* blob_ids,
                                int consistency_check, uint8_t* const* blobs_out,
                                int32_t* verdict_out, int* status_out) {
  RS2_TRY(check_value(consistency_check));  // (kNoCheck is not a value of the ABI)
  return decode_batch_host(plan, axis, n_blobs, blob_lens, counts, sliver_idx, slivers, sliver_len,
                           sliver_symbol_size, hashes, blob_ids, consistency_check, blobs_out,
                           verdict_out, status_out);
}

int rs2_set_verify_batch_budget(uint64_t bytes) {
  g_vb_budget.store(bytes ? bytes : kVerifyBatchBudget, std::memory_order_relaxed);
  return RS2_OK;
}

int rs2_verify_batch_stats(uint64_t* stats_out) {
  return read_stats(stats_out, {&g_vb_windows, &g_vb_blobs, &g_vb_rows, &g_vb_encoded});
}

int rs2_verifier_roots_device_async(rs2_verifier* v, uint32_t count, const void* d_slivers,
                                    void* d_roots, void* stream) {
  if (!v || (count && (!d_slivers || !d_roots))) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  RS2_TRY(check_symbol_ptr(d_slivers, "d_slivers"));
  RS2_TRY(check_digest_ptr(d_roots, "d_roots"));
  if (count == 0) return RS2_OK;
  HIP_TRY(hipSetDevice(v->ctx->device));
  hipStream_t st = abi_stream(stream, v->stream);
  RS2_TRY(verifier_roots(v, count, reinterpret_cast<const uint8_t*>(d_slivers),
                         reinterpret_cast<uint8_t*>(d_roots), st));
  return verifier_mark_done(v, st);
}

int rs2_verifier_recover_slivers_device_async(rs2_verifier* v, uint32_t n_slivers,
                                              const uint32_t* counts, const uint16_t* symbol_idx,
                                              const void* d_symbols, const uint8_t* expected_roots,
                                              void* d_slivers_out, void* d_roots, void* d_verdict,
                                              int* status_out, void* stream) {
  if (!v) return fail(RS2_E_INVALID_ARGUMENT, "null verifier");
  bool empty;
  RS2_TRY(batch_count(n_slivers, "slivers in a call", counts && d_slivers_out, &empty));
  if (empty) return RS2_OK;
  if (std::accumulate(counts, counts + n_slivers, size_t(0)) && (!symbol_idx || !d_symbols))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  if (expected_roots ? !d_verdict : d_verdict != nullptr)
    return fail(RS2_E_INVALID_ARGUMENT, "expected_roots and d_verdict go together");
  RS2_TRY(check_symbol_ptr(d_symbols, "d_symbols"));
  RS2_TRY(check_symbol_ptr(d_slivers_out, "d_slivers_out"));
  RS2_TRY(check_digest_ptr(d_roots, "d_roots"));
  RS2_TRY(check_digest_ptr(d_verdict, "d_verdict"));
  if (v->n <= v->k) return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "no repair symbols");
  HIP_TRY(hipSetDevice(v->ctx->device));
  // every sliver is validated before anything is enqueued
  std::vector<RecoverItem> items;
  RS2_TRY(validate_recovery(v, n_slivers, counts, symbol_idx, status_out, items));
  hipStream_t st = abi_stream(stream, v->stream);
  RS2_TRY(recover_items(v, n_slivers, items, reinterpret_cast<const uint8_t*>(d_symbols),
                        expected_roots, reinterpret_cast<uint8_t*>(d_slivers_out),
                        reinterpret_cast<uint8_t*>(d_roots), reinterpret_cast<int32_t*>(d_verdict),
                        st));
  return verifier_mark_done(v, st);
}

int rs2_recover_slivers(uint16_t n_shards, uint16_t symbol_size, int axis, uint32_t n_slivers,
                        const uint32_t* counts, const uint16_t* symbol_idx,
                        const uint8_t* const* symbols, const uint8_t* expected_roots,
                        uint8_t* const* slivers_out, uint8_t* roots_out, int32_t* verdict_out,
                        int* status_out) {
  bool empty;
  RS2_TRY(batch_count(n_slivers, "slivers in a call", counts && slivers_out, &empty));
  if (empty) return RS2_OK;
  if (expected_roots ? !verdict_out : verdict_out != nullptr)
    return fail(RS2_E_INVALID_ARGUMENT, "expected_roots and verdict_out go together");
  if (std::accumulate(counts, counts + n_slivers, size_t(0)) && (!symbol_idx || !symbols))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  VerifierLease lease;
  RS2_TRY(lease.get(n_shards, symbol_size, axis));
  rs2_verifier* v = lease.v;
  if (v->n <= v->k) return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "no repair symbols");
  std::vector<RecoverItem> items;
  RS2_TRY(validate_recovery(v, n_slivers, counts, symbol_idx, status_out, items));
  for (const RecoverItem& it : items) {
    if (!slivers_out[it.slot]) return fail(RS2_E_INVALID_ARGUMENT, "null output sliver");
    for (const auto& c : it.chosen)
      if (!symbols[it.first + c.second]) return fail(RS2_E_INVALID_ARGUMENT, "null symbol");
  }
  HIP_TRY(hipSetDevice(v->ctx->device));
  hipStream_t st = v->stream;
  const size_t s = symbol_size, K = v->k, len = K * s;
  // only the chosen symbols go up, K per accepted sliver, back to back; one H2D
  const size_t in_b = items.size() * len;
  const size_t out_b = size_t(n_slivers) * len, roots_at = (out_b + 15) / 16 * 16;
  const size_t verdict_at = roots_at + size_t(n_slivers) * 32;
  const size_t back_b = verdict_at + size_t(n_slivers) * 4;
  HIP_TRY(v->input.ensure(std::max<size_t>(in_b, 16)));
  HIP_TRY(v->sym_out.ensure(back_b));
  HIP_TRY(v->h_in.ensure(std::max<size_t>(in_b, 16)));
  HIP_TRY(v->h_out.ensure(back_b));
  std::vector<RecoverItem> part = items;
  for (size_t i = 0; i < part.size(); ++i) {
    RecoverItem& it = part[i];
    for (size_t q = 0; q < K; ++q) {
      std::memcpy(static_cast<uint8_t*>(v->h_in.p) + (i * K + q) * s,
                  symbols[it.first + it.chosen[q].second], s);
      it.chosen[q].second = uint32_t(q);
    }
    it.first = i * K;
  }
  if (in_b) HIP_TRY(hipMemcpyAsync(v->input.p, v->h_in.p, in_b, hipMemcpyHostToDevice, st));
  uint8_t* dout = v->sym_out.as<uint8_t>();
  const bool roots = roots_out || expected_roots;
  RS2_TRY(recover_items(v, n_slivers, part, v->input.as<uint8_t>(), expected_roots, dout,
                        roots ? dout + roots_at : nullptr,
                        expected_roots ? reinterpret_cast<int32_t*>(dout + verdict_at) : nullptr,
                        st));
  RS2_TRY(verifier_mark_done(v, st));
  // one D2H of slivers, roots and verdicts; slots of refused slivers are not copied out
  const uint8_t* ho = nullptr;
  RS2_TRY(download_ranges(v, {{dout, back_b}}, &ho));
  for (const RecoverItem& it : items) {
    std::memcpy(slivers_out[it.slot], ho + size_t(it.slot) * len, len);
    if (roots_out)
      std::memcpy(roots_out + size_t(it.slot) * 32, ho + roots_at + size_t(it.slot) * 32, 32);
  }
  if (verdict_out) std::memcpy(verdict_out, ho + verdict_at, size_t(n_slivers) * 4);
  return RS2_OK;
}

int rs2_recover_stats(uint64_t* stats_out) {
  return read_stats(stats_out, {&g_recover_launches, &g_recover_batched, &g_recover_single});
}

int rs2_verifier_check_recovery_symbols_device_async(rs2_verifier* v, uint32_t n_slivers,
                                                     const uint32_t* counts,
                                                     const uint16_t* target_index,
                                                     const void* d_symbols, const void* d_proofs,
                                                     const void* d_expected_roots, void* d_ok,
                                                     void* stream) {
  if (!v) return fail(RS2_E_INVALID_ARGUMENT, "null verifier");
  bool empty;
  RS2_TRY(batch_count(n_slivers, "slivers in a call", counts && target_index, &empty));
  if (empty) return RS2_OK;
  const int L = merkle_path_len(v->n);
  uint64_t total = 0;
  uint32_t max_count = 0;
  std::vector<uint32_t> per(size_t(n_slivers) * 2);
  for (uint32_t i = 0; i < n_slivers; ++i) {
    if (target_index[i] >= v->n)  // merkle.rs verify_proof: the leaf index is below n_leaves
      return fail(RS2_E_INVALID_ARGUMENT, "target index too large");
    per[2 * i] = uint32_t(total);
    per[2 * i + 1] = target_index[i];
    total += counts[i];
    max_count = std::max(max_count, counts[i]);
    if (total > 0x7FFFFFFFu) return fail(RS2_E_INVALID_ARGUMENT, "too many symbols in a call");
  }
  if (total == 0) return RS2_OK;
  if (!d_symbols || !d_expected_roots || !d_ok || (L && !d_proofs))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  RS2_TRY(check_symbol_ptr(d_symbols, "d_symbols"));
  RS2_TRY(check_digest_ptr(d_proofs, "d_proofs"));
  RS2_TRY(check_digest_ptr(d_expected_roots, "d_expected_roots"));
  RS2_TRY(check_digest_ptr(d_ok, "d_ok"));
  HIP_TRY(hipSetDevice(v->ctx->device));
  hipStream_t st = abi_stream(stream, v->stream);
  HIP_TRY(v->done.wait_on(st));
  HIP_TRY(v->sym_digests.ensure(size_t(total) * 32));
  HIP_TRY(v->per_sliver.ensure(per.size() * 4));
  RS2_TRY(upload_pieces(v->ctx, v->per_sliver.p, per.data(), per.size() * 4, st));
  HIP_TRY(hash_symbols(d_symbols, int64_t(total), int(v->s), v->sym_digests.p, st));
  HIP_TRY(rs2k_launch_recovery_proof_check(
      v->sym_digests.as<uint8_t>(), v->per_sliver.as<uint32_t>(), int(n_slivers), max_count,
      uint32_t(total), reinterpret_cast<const uint8_t*>(d_proofs), L,
      reinterpret_cast<const uint8_t*>(d_expected_roots), reinterpret_cast<uint8_t*>(d_ok), st));
  return verifier_mark_done(v, st);
}

int rs2_check_recovery_symbols(uint16_t n_shards, uint16_t symbol_size, int axis,
                               uint32_t n_slivers, const uint32_t* counts,
                               const uint16_t* target_index, const uint8_t* symbols,
                               const uint8_t* proofs, const uint8_t* expected_roots,
                               uint8_t* ok_out) {
  if (n_slivers == 0) return RS2_OK;
  if (!counts || !target_index) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  size_t total = 0;
  for (uint32_t i = 0; i < n_slivers; ++i) total += counts[i];
  VerifierLease lease;
  RS2_TRY(lease.get(n_shards, symbol_size, axis));
  rs2_verifier* v = lease.v;
  const size_t L = size_t(merkle_path_len(n_shards));
  if (total && (!symbols || !expected_roots || !ok_out || (L && !proofs)))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(v->ctx->device));
  hipStream_t st = v->stream;
  // symbols, proofs and expected roots through one pinned buffer: one H2D
  const size_t sym_b = total * symbol_size, prf_at = (sym_b + 15) / 16 * 16;
  const size_t exp_at = prf_at + total * L * 32, ok_at = exp_at + total * 32;
  const size_t all_b = ok_at + (total + 15) / 16 * 16;
  HIP_TRY(v->input.ensure(std::max<size_t>(all_b, 16)));
  HIP_TRY(v->h_in.ensure(std::max<size_t>(ok_at, 16)));
  HIP_TRY(v->h_out.ensure(std::max<size_t>(total, 16)));
  uint8_t* hi = static_cast<uint8_t*>(v->h_in.p);
  if (total) {
    std::memcpy(hi, symbols, sym_b);
    if (L) std::memcpy(hi + prf_at, proofs, total * L * 32);
    std::memcpy(hi + exp_at, expected_roots, total * 32);
    HIP_TRY(hipMemcpyAsync(v->input.p, hi, ok_at, hipMemcpyHostToDevice, st));
  }
  uint8_t* d = v->input.as<uint8_t>();
  RS2_TRY(rs2_verifier_check_recovery_symbols_device_async(v, n_slivers, counts, target_index, d,
                                                           d + prf_at, d + exp_at, d + ok_at,
                                                           nullptr));
  if (total) {
    const uint8_t* ho = nullptr;
    RS2_TRY(download_ranges(v, {{d + ok_at, total}}, &ho));
    std::memcpy(ok_out, ho, total);
  }
  return RS2_OK;
}

int rs2_verifier_recovery_symbols_device_async(rs2_verifier* v, uint32_t count,
                                               const void* d_slivers,
                                               const uint16_t* target_sliver_index,
                                               void* d_symbols, void* d_proofs, void* d_nodes,
                                               void* stream) {
  if (!v || (count && (!d_slivers || !target_sliver_index || !d_symbols || !d_proofs)))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  RS2_TRY(check_symbol_ptr(d_slivers, "d_slivers"));
  RS2_TRY(check_symbol_ptr(d_symbols, "d_symbols"));
  RS2_TRY(check_digest_ptr(d_proofs, "d_proofs"));
  RS2_TRY(check_digest_ptr(d_nodes, "d_nodes"));
  for (uint32_t i = 0; i < count; ++i)
    if (target_sliver_index[i] >= v->n)  // slivers.rs check_index -> RecoverySymbolError::IndexTooLarge
      return fail(RS2_E_INVALID_ARGUMENT, "target index too large");
  if (count == 0) return RS2_OK;
  HIP_TRY(hipSetDevice(v->ctx->device));
  hipStream_t st = abi_stream(stream, v->stream);
  RS2_TRY(verifier_leaves(v, count, reinterpret_cast<const uint8_t*>(d_slivers), st));
  const int64_t n = v->n, nn = int64_t(merkle_n_nodes(uint64_t(n)));
  uint8_t* nodes = reinterpret_cast<uint8_t*>(d_nodes);
  if (!nodes) {
    HIP_TRY(v->nodes.ensure(size_t(count) * nn * 32));
    nodes = v->nodes.as<uint8_t>();
  }
  HIP_TRY(v->roots.ensure(size_t(count) * 32));
  HIP_TRY(rs2k_launch_merkle_trees(v->leaves.as<uint8_t>(), int(n), int(count), 0, n * 32, 32, 0, 0,
                                   v->roots.as<uint8_t>(), 32, st, nodes, nn * 32));
  // the targets go up through a pinned upload slot (no host copy to keep alive); the device
  // buffer is rewritten in stream order after the previous call's gather (verifier calls on
  // different streams are ordered by verifier_mark_done)
  v->targets_h.assign(target_sliver_index, target_sliver_index + count);
  HIP_TRY(v->targets.ensure(size_t(count) * 2));
  HIP_TRY(v->ctx->upload(v->targets.p, v->targets_h.data(), size_t(count) * 2, st));
  HIP_TRY(rs2k_launch_proof_gather(reinterpret_cast<const uint8_t*>(d_slivers),
                                   v->repair.as<uint8_t>(), int(n), int(v->k), int(v->s), nodes,
                                   nn * 32, v->targets.as<uint16_t>(), int(count),
                                   merkle_path_len(n), reinterpret_cast<uint8_t*>(d_symbols),
                                   reinterpret_cast<uint8_t*>(d_proofs), st));
  return verifier_mark_done(v, st);
}

int rs2_merkle_tree_shape(uint32_t n_leaves, uint32_t* path_len, uint64_t* n_nodes) {
  if (path_len) *path_len = uint32_t(merkle_path_len(n_leaves));
  if (n_nodes) *n_nodes = merkle_n_nodes(n_leaves);
  return RS2_OK;
}

int rs2_recovery_symbols(uint16_t n_shards, uint16_t symbol_size, int axis, uint32_t count,
                         const uint8_t* const* slivers, const uint64_t* sliver_len,
                         const uint16_t* target_sliver_index, uint8_t* symbols_out,
                         uint8_t* proofs_out) {
  if (count && (!slivers || !sliver_len || !target_sliver_index || !symbols_out || !proofs_out))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  VerifierLease lease;
  RS2_TRY(lease.get(n_shards, symbol_size, axis));
  rs2_verifier* v = lease.v;
  RS2_TRY(check_host_slivers(v, count, slivers, sliver_len));
  // every argument checked before any work is queued (a target is remote input on a node)
  for (uint32_t i = 0; i < count; ++i)
    if (target_sliver_index[i] >= n_shards)  // slivers.rs check_index -> IndexTooLarge
      return fail(RS2_E_INVALID_ARGUMENT, "target index too large");
  if (count == 0) return RS2_OK;
  HIP_TRY(hipSetDevice(v->ctx->device));
  const int L = merkle_path_len(n_shards);
  const size_t sym_b = size_t(count) * symbol_size, prf_b = size_t(count) * L * 32;
  HIP_TRY(v->sym_out.ensure(sym_b));
  HIP_TRY(v->proof_out.ensure(size_t(count) * std::max(L, 1) * 32));
  RS2_TRY(upload_host_slivers(v, count, slivers, sym_b + prf_b));
  RS2_TRY(rs2_verifier_recovery_symbols_device_async(v, count, v->input.p, target_sliver_index,
                                                     v->sym_out.p, v->proof_out.p, nullptr, nullptr));
  const uint8_t* ho = nullptr;
  RS2_TRY(download_ranges(v, {{v->sym_out.p, sym_b}, {v->proof_out.p, prf_b}}, &ho));
  std::memcpy(symbols_out, ho, sym_b);
  if (L) std::memcpy(proofs_out, ho + sym_b, prf_b);
  return RS2_OK;
}

int rs2_verifier_recovery_symbols_multi_device_async(
    rs2_verifier* v, uint32_t n_slivers, const void* d_slivers, const uint32_t* target_counts,
    const uint16_t* target_sliver_index, int trees, void* d_nodes, void* d_symbols, void* d_proofs,
    void* stream) {
  if (!v) return fail(RS2_E_INVALID_ARGUMENT, "null verifier");
  if (trees != RS2_TREES_BUILD && trees != RS2_TREES_CACHED)
    return fail(RS2_E_INVALID_ARGUMENT, "trees must be RS2_TREES_BUILD or RS2_TREES_CACHED");
  if (n_slivers == 0) return RS2_OK;
  if (!d_slivers || !target_counts) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  RS2_TRY(check_symbol_ptr(d_slivers, "d_slivers"));
  RS2_TRY(check_symbol_ptr(d_symbols, "d_symbols"));
  RS2_TRY(check_digest_ptr(d_proofs, "d_proofs"));
  RS2_TRY(check_digest_ptr(d_nodes, "d_nodes"));
  // every argument checked and the whole call planned before anything is enqueued (a target is
  // remote input on a node)
  SymbolRequestPlan plan;
  RS2_TRY(plan_symbol_requests(v->n, v->k, v->s, n_slivers, target_counts, target_sliver_index,
                               trees, d_nodes != nullptr,
                               g_sym_budget.load(std::memory_order_relaxed), plan));
  if (plan.total && (!d_symbols || (plan.path_len && !d_proofs)))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(v->ctx->device));
  hipStream_t st = abi_stream(stream, v->stream);
  RS2_TRY(symbol_request_windows(v, plan, target_counts, trees,
                                 reinterpret_cast<const uint8_t*>(d_slivers),
                                 reinterpret_cast<uint8_t*>(d_nodes),
                                 reinterpret_cast<uint8_t*>(d_symbols),
                                 reinterpret_cast<uint8_t*>(d_proofs), st));
  return verifier_mark_done(v, st);
}

int rs2_recovery_symbols_multi(uint16_t n_shards, uint16_t symbol_size, int axis,
                               uint32_t n_slivers, const uint8_t* const* slivers,
                               const uint64_t* sliver_len, const uint32_t* target_counts,
                               const uint16_t* target_sliver_index, uint8_t* symbols_out,
                               uint8_t* proofs_out) {
  bool empty;
  RS2_TRY(batch_count(n_slivers, "slivers in a call", slivers && sliver_len && target_counts, &empty));
  if (empty) return RS2_OK;
  VerifierLease lease;
  RS2_TRY(lease.get(n_shards, symbol_size, axis));
  rs2_verifier* v = lease.v;
  RS2_TRY(check_host_slivers(v, n_slivers, slivers, sliver_len));
  uint64_t total = 0;
  for (uint32_t i = 0; i < n_slivers; ++i) {
    total += target_counts[i];
    if (total > 0x7FFFFFFFu) return fail(RS2_E_INVALID_ARGUMENT, "too many requests in a call");
  }
  if (total && !target_sliver_index) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  for (uint64_t j = 0; j < total; ++j)
    if (target_sliver_index[j] >= n_shards)  // slivers.rs check_index -> IndexTooLarge
      return fail(RS2_E_INVALID_ARGUMENT, "target index too large");
  const size_t L = size_t(merkle_path_len(n_shards));
  if (total && (!symbols_out || (L && !proofs_out)))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  if (total == 0) return RS2_OK;  // no trees to hand out: nothing to do
  HIP_TRY(hipSetDevice(v->ctx->device));
  const size_t sym_b = size_t(total) * symbol_size, prf_b = size_t(total) * L * 32;
  HIP_TRY(v->sym_out.ensure(sym_b));
  HIP_TRY(v->proof_out.ensure(std::max<size_t>(prf_b, 32)));
  RS2_TRY(upload_host_slivers(v, n_slivers, slivers, sym_b + prf_b));
  RS2_TRY(rs2_verifier_recovery_symbols_multi_device_async(
      v, n_slivers, v->input.p, target_counts, target_sliver_index, RS2_TREES_BUILD, nullptr,
      v->sym_out.p, v->proof_out.p, nullptr));
  const uint8_t* ho = nullptr;
  RS2_TRY(download_ranges(v, {{v->sym_out.p, sym_b}, {v->proof_out.p, prf_b}}, &ho));
  std::memcpy(symbols_out, ho, sym_b);
  if (L) std::memcpy(proofs_out, ho + sym_b, prf_b);
  return RS2_OK;
}

int rs2_set_recovery_symbols_budget(uint64_t bytes) {
  g_sym_budget.store(bytes ? bytes : kSymbolsBudget, std::memory_order_relaxed);
  return RS2_OK;
}

int rs2_recovery_symbols_stats(uint64_t* stats_out) {
  return read_stats(stats_out, {&g_sym_windows, &g_sym_expanded, &g_sym_built, &g_sym_cached,
                                &g_sym_requests});
}

int rs2_merkle_proof_roots(uint32_t count, const uint8_t* leaves, uint32_t leaf_len,
                           const uint32_t* leaf_index, const uint8_t* paths, uint32_t path_len,
                           uint8_t* roots_out) {
  if (count && (!leaves || !leaf_index || !roots_out || (path_len && !paths)))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  if (leaf_len % 2) return fail(RS2_E_INVALID_ARGUMENT, "leaf length must be even (symbols are)");
  if (count == 0) return RS2_OK;
  Context* ctx = nullptr;
  RS2_TRY(get_context(&ctx));
  hipStream_t st = ctx->util_stream;
  DevBuf dl, dd, di, dp, dr;
  HIP_TRY(dl.ensure(std::max<size_t>(size_t(count) * leaf_len, 16)));
  HIP_TRY(dd.ensure(size_t(count) * 32));
  HIP_TRY(di.ensure(size_t(count) * 4));
  HIP_TRY(dp.ensure(std::max<size_t>(size_t(count) * path_len * 32, 16)));
  HIP_TRY(dr.ensure(size_t(count) * 32));
  if (leaf_len)
    HIP_TRY(hipMemcpyAsync(dl.p, leaves, size_t(count) * leaf_len, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(di.p, leaf_index, size_t(count) * 4, hipMemcpyHostToDevice, st));
  if (path_len)
    HIP_TRY(hipMemcpyAsync(dp.p, paths, size_t(count) * path_len * 32, hipMemcpyHostToDevice, st));
  HIP_TRY(hash_symbols(dl.p, count, int(leaf_len), dd.p, st));
  HIP_TRY(rs2k_launch_proof_roots(dd.as<uint8_t>(), di.as<uint32_t>(), dp.as<uint8_t>(),
                                  int(path_len), int(count), dr.as<uint8_t>(), st));
  HIP_TRY(hipMemcpyAsync(roots_out, dr.p, size_t(count) * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return RS2_OK;
}

int rs2_sliver_merkle_roots(uint16_t n_shards, uint16_t symbol_size, int axis, uint32_t count,
                            const uint8_t* const* slivers, const uint64_t* sliver_len,
                            uint8_t* roots_out) {
  if (count && (!slivers || !sliver_len || !roots_out))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  VerifierLease lease;
  RS2_TRY(lease.get(n_shards, symbol_size, axis));
  rs2_verifier* v = lease.v;
  RS2_TRY(check_host_slivers(v, count, slivers, sliver_len));
  if (count == 0) return RS2_OK;
  HIP_TRY(hipSetDevice(v->ctx->device));
  HIP_TRY(v->roots.ensure(size_t(count) * 32));
  RS2_TRY(upload_host_slivers(v, count, slivers, size_t(count) * 32));
  RS2_TRY(rs2_verifier_roots_device_async(v, count, v->input.p, v->roots.p, nullptr));
  const uint8_t* ho = nullptr;
  RS2_TRY(download_ranges(v, {{v->roots.p, size_t(count) * 32}}, &ho));
  std::memcpy(roots_out, ho, size_t(count) * 32);
  return RS2_OK;
}

int rs2_sliver_merkle_root(uint16_t n_shards, uint16_t symbol_size, int axis, const uint8_t* sliver,
                           uint64_t sliver_len, uint8_t root_out[32]) {
  if (!sliver || !root_out || symbol_size == 0) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  return rs2_sliver_merkle_roots(n_shards, symbol_size, axis, 1, &sliver, &sliver_len, root_out);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// mixed sliver verification: slivers that share only n_shards, a symbol size per sliver
// ---------------------------------------------------------------------------------------------
namespace {
constexpr uint64_t kVerifyMixedBudget = uint64_t(256) << 20;
std::atomic<uint64_t> g_vm_budget{kVerifyMixedBudget};
std::atomic<uint64_t> g_vm_windows{0}, g_vm_grouped{0}, g_vm_single{0}, g_vm_groups{0},
    g_vm_launches{0};
// Groups of one window: what keeps its job table within one upload slot, so the compute launches
// of a window (RS2_VERIFY_MIXED_WINDOW_LAUNCHES) never depend on how many sizes it holds.
constexpr uint32_t kMixedWindowGroups = RS2_VERIFY_MIXED_WINDOW_GROUPS;
static_assert(kMixedWindowGroups <= kBatchChunkJobs, "a window's job table outgrows an upload slot");

hipError_t launch_encode_groups(int C, const CodecJobBatch* d_jobs, const uint32_t* d_tiles,
                                int n_jobs, int n_tiles, int n_z, int mode, hipStream_t st) {
  switch (C) {
#define RS2_GROUPS_CASE(CC) \
  case CC: return rs2k_launch_encode_groups_##CC(d_jobs, d_tiles, n_jobs, n_tiles, n_z, mode, st);
    RS2_GROUPS_CASE(1)
    RS2_GROUPS_CASE(2)
    RS2_GROUPS_CASE(4)
    RS2_GROUPS_CASE(8)
    RS2_GROUPS_CASE(16)
    RS2_GROUPS_CASE(32)
    RS2_GROUPS_CASE(64)
    RS2_GROUPS_CASE(128)
    RS2_GROUPS_CASE(256)
    RS2_GROUPS_CASE(512)
#undef RS2_GROUPS_CASE
    default: return hipErrorInvalidValue;
  }
}

// The codes of both axes, planned once per checker (again only when the block limit changed):
// host arithmetic only.
int checker_codes(rs2_sliver_checker* c) {
  for (int a = 0; a < 2; ++a) {
    SliverAxisCode& code = c->codes[a];
    if (code.n == c->n && code.block_max == block_max()) continue;
    RS2_TRY(plan_sliver_axis(c->n, a, code));
    c->bound[a] = false;
  }
  return RS2_OK;
}

// A freshly planned code's device side: its blocks get their transform tables, and its mixing
// tables go up on st (calls on other streams are ordered behind st by the checker's `done`).
int checker_bind(rs2_sliver_checker* c, hipStream_t st) {
  for (int a = 0; a < 2; ++a) {
    SliverAxisCode& code = c->codes[a];
    if (c->bound[a] || !code.batchable) continue;
    const PlannedJob& t = code.tmpl;
    CodecJobBatch& j = code.job;
    for (int b = 0; b < j.n_in; ++b) {
      j.in[b].sd_tab = c->ctx->stream(t.C, t.in_sd[size_t(b)], t.ppw);
      if (!j.in[b].sd_tab) return fail(RS2_E_DEVICE, "table upload failed");
      j.in[b].zero_first = group0_zero(t.C, t.in_sd[size_t(b)], t.ppw);
    }
    for (int o = 0; o < j.n_out; ++o) {
      j.out[o].sd_tab = c->ctx->stream(t.C, t.out_sd[size_t(o)], t.ppw);
      if (!j.out[o].sd_tab) return fail(RS2_E_DEVICE, "table upload failed");
      j.out[o].zero_first = group0_zero(t.C, t.out_sd[size_t(o)], t.ppw);
    }
    j.mix_tab = nullptr;
    if (!code.mix.empty()) {
      HIP_TRY(c->mix[a].ensure(code.mix.size() * 2));
      RS2_TRY(upload_pieces(c->ctx, c->mix[a].p, code.mix.data(), code.mix.size() * 2, st));
      j.mix_tab = c->mix[a].as<uint16_t>();
    }
    c->bound[a] = true;
  }
  return RS2_OK;
}

// Where a window's tables lie in the checker's table buffer (every part 16-byte aligned).
struct MixedTables {
  size_t slots = 0, groups = 0, jobs = 0, tiles[2] = {0, 0}, offs = 0, slot_of = 0, expected = 0,
         bytes = 0;
};
MixedTables mixed_tables(const rs2_sliver_checker* c, const SliverWindow& w, bool verdicts) {
  MixedTables t;
  size_t at = 0;
  auto take = [&](size_t n) {
    const size_t here = at;
    at += (n + 15) / 16 * 16;
    return here;
  };
  const size_t ne = size_t(w.axis_groups[0]) + w.axis_groups[1];
  t.slots = take((size_t(w.n_slots) + 1) * sizeof(SliverSlot));
  t.groups = take((ne + 1) * sizeof(SliverLeafGroup));
  t.jobs = take(ne * sizeof(CodecJobBatch));
  size_t n_offs = 0;
  for (int a = 0; a < 2; ++a) {
    t.tiles[a] = take(w.tiles[a].size() * 4);
    n_offs += size_t(w.axis_groups[a]) * c->codes[a].tmpl.offs.size();
  }
  t.offs = take(n_offs * 8);
  t.slot_of = take(size_t(w.count) * 4);
  t.expected = take(verdicts ? size_t(w.count) * 32 : 0);
  t.bytes = std::max<size_t>(at, 16);
  return t;
}

// Window w's slot, leaf-group, job, tile and position-offset tables into h_tab (laid out by t;
// d_tab: where they will lie on the device).  src(i): the device address of the caller's sliver i.
// *chunks_out: the 4 KiB chunks of the window's gather launch.
template <class SrcF>
int pack_group_tables(const rs2_sliver_checker* c, const SliverWindow& w, SrcF src,
                      const MixedTables& t, uint8_t* h_tab, const uint8_t* d_tab, uint8_t* gath,
                      uint8_t* rep, uint64_t* chunks_out) {
  const int64_t n = c->n;
  // slots: where each sliver comes from and goes to, and its chunks of the gather
  SliverSlot* slots = reinterpret_cast<SliverSlot*>(h_tab + t.slots);
  uint64_t chunks = 0;
  for (const SliverGroup& g : w.groups) {
    const uint64_t len = uint64_t(g.k) * g.s;
    for (uint32_t q = 0; q < g.count; ++q) {
      SliverSlot& sl = slots[g.first_slot + q];
      sl.src = src(w.perm[g.first_slot + q]);
      sl.dst_off = g.gather_off + q * len;
      sl.len = uint32_t(len);
      sl.chunk0 = uint32_t(chunks);
      chunks += (len + 4095) / 4096;
      if (chunks > 0x7FFFFFFFu) return fail(RS2_E_UNSUPPORTED, "window exceeds the launch grid");
    }
  }
  slots[w.n_slots].chunk0 = uint32_t(chunks);
  *chunks_out = chunks;
  // eligible groups: leaf table, jobs, tiles, position offsets
  SliverLeafGroup* lg = reinterpret_cast<SliverLeafGroup*>(h_tab + t.groups);
  CodecJobBatch* jobs = reinterpret_cast<CodecJobBatch*>(h_tab + t.jobs);
  int64_t* offs = reinterpret_cast<int64_t*>(h_tab + t.offs);
  const int64_t* d_offs = reinterpret_cast<const int64_t*>(d_tab + t.offs);
  const uint32_t ne = w.axis_groups[0] + w.axis_groups[1];
  size_t off_at = 0;
  for (uint32_t p = 0; p < ne; ++p) {
    const SliverGroup& g = w.groups[p];
    const SliverAxisCode& code = c->codes[g.axis];
    const PlannedJob& tp = code.tmpl;
    const int64_t s = g.s, k = g.k;
    lg[p] = {gath + g.gather_off, rep + g.repair_off, g.first_slot, g.count, g.k, g.s};
    CodecJobBatch j = code.job;
    j.symbol_size = int32_t(s);
    j.n_pairs = int32_t((s + 3) / 4);
    j.pairs_span = g.pairs_span;
    j.n_lines = int32_t(g.count);
    for (int b = 0; b < j.n_in; ++b) {
      j.in[b].base = gath + g.gather_off;
      j.in[b].line_stride = k * s;
      j.in[b].pos_off = d_offs + off_at + tp.in_off(b);
    }
    for (int o = 0; o < j.n_out; ++o) {
      j.out[o].base = rep + g.repair_off;
      j.out[o].line_stride = (n - k) * s;
      j.out[o].pos_off = d_offs + off_at + tp.out_off(o);
    }
    jobs[p] = j;
    for (size_t q = 0; q < tp.offs.size(); ++q)
      offs[off_at + q] = tp.offs[q] < 0 ? int64_t(-1) : tp.offs[q] * s;
    off_at += tp.offs.size();
  }
  lg[ne].first_slot = w.n_eligible_slots;
  for (int a = 0; a < 2; ++a)
    std::memcpy(h_tab + t.tiles[a], w.tiles[a].data(), w.tiles[a].size() * 4);
  return RS2_OK;
}

// The expansion of window w from its uploaded tables, on st: the gather of its slots and the
// encode launch of each axis with eligible groups.  *launches counts them.
int launch_group_expand(const rs2_sliver_checker* c, const SliverWindow& w, const MixedTables& t,
                        const uint8_t* d_tab, uint8_t* gath, uint64_t chunks, hipStream_t st,
                        uint64_t* launches) {
  if (w.n_slots) {
    HIP_TRY(rs2k_launch_sliver_gather(reinterpret_cast<const SliverSlot*>(d_tab + t.slots),
                                      int(w.n_slots), int64_t(chunks), gath, st));
    ++*launches;
  }
  for (int a = 0; a < 2; ++a) {
    if (!w.axis_groups[a]) continue;
    const PlannedJob& tp = c->codes[a].tmpl;
    HIP_TRY(launch_encode_groups(
        tp.C, reinterpret_cast<const CodecJobBatch*>(d_tab + t.jobs) + w.axis_first[a],
        reinterpret_cast<const uint32_t*>(d_tab + t.tiles[a]), int(w.axis_groups[a]),
        int(w.tiles[a].back()), tp.n_z, tp.mode, st));
    ++*launches;
  }
  return RS2_OK;
}

// Run a planned call on st.  src(i): the device address of the caller's sliver i (accepted ones
// only).  expected / d_roots / d_verdict are indexed by the caller's sliver.  Every buffer is
// sized for the call's largest window before the first window runs.  before(w) runs on st ahead
// of window w's own work (the mixed recovery decodes the window's slivers there).
inline int no_window_hook(const SliverWindow&) { return RS2_OK; }
template <class SrcF, class BeforeF = int (*)(const SliverWindow&)>
int checker_run(rs2_sliver_checker* c, const SliverGroupsPlan& plan, SrcF src,
                const uint8_t* expected, uint8_t* d_roots, int32_t* d_verdict, hipStream_t st,
                BeforeF before = no_window_hook) {
  Context* ctx = c->ctx;
  const int64_t n = c->n;
  // a previous call on another stream still owns the scratch buffers and tables
  HIP_TRY(c->done.wait_on(st));
  if (plan.accepted) RS2_TRY(checker_bind(c, st));
  uint64_t max_gather = 0, max_repair = 0;
  uint32_t max_slots = 0, max_elig = 0;
  size_t max_tab = 0;
  for (const SliverWindow& w : plan.windows) {
    max_gather = std::max(max_gather, w.gather_bytes);
    max_repair = std::max(max_repair, w.repair_bytes);
    max_slots = std::max(max_slots, w.n_slots);
    max_elig = std::max(max_elig, w.n_eligible_slots);
    max_tab = std::max(max_tab, mixed_tables(c, w, d_verdict != nullptr).bytes);
  }
  HIP_TRY(c->gathered.ensure(std::max<uint64_t>(max_gather, 16)));
  HIP_TRY(c->repair.ensure(std::max<uint64_t>(max_repair, 16)));
  HIP_TRY(c->leaves.ensure(std::max<size_t>(size_t(max_elig) * size_t(n) * 32, 16)));
  HIP_TRY(c->slot_roots.ensure(std::max<size_t>(size_t(max_slots) * 32, 16)));
  HIP_TRY(c->tables.ensure(max_tab));
  uint8_t* const gath = c->gathered.as<uint8_t>();
  uint8_t* const rep = c->repair.as<uint8_t>();
  uint8_t* const d_tab = c->tables.as<uint8_t>();
  std::vector<uint8_t> h_tab;
  for (const SliverWindow& w : plan.windows) {
    RS2_TRY(before(w));
    const MixedTables t = mixed_tables(c, w, d_verdict != nullptr);
    h_tab.assign(t.bytes, 0);
    uint64_t chunks = 0;
    RS2_TRY(pack_group_tables(c, w, src, t, h_tab.data(), d_tab, gath, rep, &chunks));
    const uint32_t ne = w.axis_groups[0] + w.axis_groups[1];
    uint32_t* slot_of = reinterpret_cast<uint32_t*>(h_tab.data() + t.slot_of);
    std::fill(slot_of, slot_of + w.count, kSliverSkipped);
    for (uint32_t sl = 0; sl < w.n_slots; ++sl) slot_of[w.perm[sl] - w.first] = sl;
    if (d_verdict)
      std::memcpy(h_tab.data() + t.expected, expected + size_t(w.first) * 32, size_t(w.count) * 32);
    RS2_TRY(upload_pieces(ctx, d_tab, h_tab.data(), t.bytes, st));
    uint64_t launches = 0;
    RS2_TRY(launch_group_expand(c, w, t, d_tab, gath, chunks, st, &launches));
    if (w.n_eligible_slots) {
      HIP_TRY(rs2k_launch_leaf_hash_groups(reinterpret_cast<const SliverLeafGroup*>(d_tab + t.groups),
                                           int(ne), int(w.n_eligible_slots), int(n),
                                           c->leaves.as<uint8_t>(), st));
      HIP_TRY(rs2k_launch_merkle_trees(c->leaves.as<uint8_t>(), int(n), int(w.n_eligible_slots), 0,
                                       n * 32, 32, 0, 0, c->slot_roots.as<uint8_t>(), 32, st));
      launches += 2;
    }
    // the other groups: the per-size path on the same stream, from their gathered copies
    for (size_t p = ne; p < w.groups.size(); ++p) {
      const SliverGroup& g = w.groups[p];
      rs2_verifier* v = c->single;
      v->s = uint16_t(g.s);
      v->k = uint16_t(g.k);
      v->axis = g.axis;
      RS2_TRY(verifier_roots(v, g.count, gath + g.gather_off,
                             c->slot_roots.as<uint8_t>() + size_t(g.first_slot) * 32, st));
      RS2_TRY(verifier_mark_done(v, st));
    }
    if (d_roots || d_verdict) {
      HIP_TRY(rs2k_launch_sliver_finish(
          c->slot_roots.as<uint8_t>(), reinterpret_cast<const uint32_t*>(d_tab + t.slot_of),
          int(w.count), d_verdict ? d_tab + t.expected : nullptr,
          d_roots ? d_roots + size_t(w.first) * 32 : nullptr,
          d_verdict ? d_verdict + w.first : nullptr, st));
      ++launches;
    }
    g_vm_windows.fetch_add(1, std::memory_order_relaxed);
    g_vm_grouped.fetch_add(w.n_eligible_slots, std::memory_order_relaxed);
    g_vm_single.fetch_add(w.n_slots - w.n_eligible_slots, std::memory_order_relaxed);
    g_vm_groups.fetch_add(w.groups.size(), std::memory_order_relaxed);
    g_vm_launches.fetch_add(launches, std::memory_order_relaxed);
  }
  HIP_TRY(c->done.record(st));
  return RS2_OK;
}

// The whole-call rules both forms share; *empty: nothing to do (RS2_OK).
int check_mixed_call(uint32_t n_slivers, bool arrays, const void* expected, const void* verdict,
                     bool* empty) {
  RS2_TRY(batch_count(n_slivers, "slivers in a call", arrays, empty));
  if (*empty) return RS2_OK;
  if (expected ? !verdict : verdict != nullptr)
    return fail(RS2_E_INVALID_ARGUMENT, "expected_roots and the verdicts go together");
  return RS2_OK;
}

// A pooled checker for one host-buffer call (Context::checker_pool), as VerifierLease.
struct CheckerLease {
  Context* ctx = nullptr;
  rs2_sliver_checker* c = nullptr;
  CheckerLease() = default;
  CheckerLease(const CheckerLease&) = delete;
  CheckerLease& operator=(const CheckerLease&) = delete;
  int get(uint16_t n_shards) {
    RS2_TRY(get_context(&ctx));
    {
      std::lock_guard<std::mutex> lk(ctx->pool_mu);
      auto& free_ = ctx->checker_pool[int(n_shards)];
      if (!free_.empty()) {
        c = free_.back();
        free_.pop_back();
        return RS2_OK;
      }
    }
    return rs2_sliver_checker_create(n_shards, &c);
  }
  ~CheckerLease() {
    if (!c) return;
    (void)hipStreamSynchronize(c->stream);
    (void)c->done.sync();
    {
      std::lock_guard<std::mutex> lk(ctx->pool_mu);
      auto& free_ = ctx->checker_pool[int(c->n)];
      if (free_.size() < Context::kPoolKeep) {
        free_.push_back(c);
        return;
      }
    }
    rs2_sliver_checker_destroy(c);
  }
};
}  // namespace

extern "C" {

int rs2_sliver_checker_create(uint16_t n_shards, rs2_sliver_checker** out) {
  if (!out) return fail(RS2_E_INVALID_ARGUMENT, "null checker pointer");
  *out = nullptr;
  uint16_t kp, ks;
  RS2_TRY(rs2_source_symbols_for_n_shards(n_shards, &kp, &ks));
  if (n_shards > kMaxShards) return fail(RS2_E_UNSUPPORTED, "n_shards above 65535");
  Context* ctx = nullptr;
  RS2_TRY(get_context(&ctx));
  auto c = std::make_unique<rs2_sliver_checker>();
  c->ctx = ctx;
  c->n = n_shards;
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  // the per-size path's verifier, re-pointed at each group it runs
  RS2_TRY(rs2_verifier_create(n_shards, 2, RS2_AXIS_PRIMARY, &c->single));
  *out = c.release();
  return RS2_OK;
}

void rs2_sliver_checker_destroy(rs2_sliver_checker* c) {
  if (!c) return;
  (void)hipSetDevice(c->ctx->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  (void)c->done.sync();  // work queued on a caller's stream
  if (c->single) rs2_verifier_destroy(c->single);
  const Quiesced quiesced;
  delete c;
}

int rs2_sliver_checker_verify_device_async(rs2_sliver_checker* c, uint32_t n_slivers,
                                           const uint8_t* axis, const uint16_t* symbol_size,
                                           const void* d_slivers_base, const uint64_t* sliver_off,
                                           const uint8_t* expected_roots, void* d_roots,
                                           void* d_verdict, int* status_out, void* stream) {
  if (!c) return fail(RS2_E_INVALID_ARGUMENT, "null checker");
  bool empty;
  RS2_TRY(check_mixed_call(n_slivers, axis && symbol_size && d_slivers_base && sliver_off,
                           expected_roots, d_verdict, &empty));
  if (empty) return RS2_OK;
  RS2_TRY(check_symbol_ptr(d_slivers_base, "d_slivers_base"));
  RS2_TRY(check_digest_ptr(d_roots, "d_roots"));
  RS2_TRY(check_digest_ptr(d_verdict, "d_verdict"));
  HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = abi_stream(stream, c->stream);
  // every sliver is validated, and the call planned, before anything is enqueued
  RS2_TRY(checker_codes(c));
  SliverGroupsPlan plan;
  RS2_TRY(plan_sliver_groups(c->codes, n_slivers, axis, symbol_size, sliver_off, nullptr, nullptr,
                             g_vm_budget.load(std::memory_order_relaxed), kMixedWindowGroups,
                             status_out, plan));
  const uint8_t* base = reinterpret_cast<const uint8_t*>(d_slivers_base);
  return checker_run(c, plan, [&](uint32_t i) { return base + sliver_off[i]; }, expected_roots,
                     reinterpret_cast<uint8_t*>(d_roots), reinterpret_cast<int32_t*>(d_verdict), st);
}

int rs2_verify_slivers_mixed(uint16_t n_shards, uint32_t n_slivers, const uint8_t* axis,
                             const uint16_t* symbol_size, const uint8_t* const* slivers,
                             const uint64_t* sliver_len, const uint8_t* expected_roots,
                             uint8_t* roots_out, int32_t* verdict_out, int* status_out) {
  bool empty;
  RS2_TRY(check_mixed_call(n_slivers, axis && symbol_size && slivers && sliver_len, expected_roots,
                           verdict_out, &empty));
  if (empty) return RS2_OK;
  CheckerLease lease;
  RS2_TRY(lease.get(n_shards));
  rs2_sliver_checker* c = lease.c;
  HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->stream;
  RS2_TRY(checker_codes(c));
  SliverGroupsPlan plan;
  RS2_TRY(plan_sliver_groups(c->codes, n_slivers, axis, symbol_size, nullptr, slivers, sliver_len,
                             g_vm_budget.load(std::memory_order_relaxed), kMixedWindowGroups,
                             status_out, plan));
  // the accepted slivers back to back through pinned staging: one H2D
  std::vector<uint64_t> off(n_slivers, 0);
  std::vector<uint8_t> accepted(n_slivers, 0);
  uint64_t in_b = 0;
  for (const SliverWindow& w : plan.windows)
    for (uint32_t i : w.perm) accepted[i] = 1;
  for (uint32_t i = 0; i < n_slivers; ++i) {
    if (!accepted[i]) continue;
    off[i] = in_b;
    in_b += sliver_len[i];
  }
  const size_t roots_b = size_t(n_slivers) * 32, back_b = roots_b + size_t(n_slivers) * 4;
  HIP_TRY(c->input.ensure(std::max<uint64_t>(in_b, 16)));
  HIP_TRY(c->h_in.ensure(std::max<uint64_t>(in_b, 16)));
  HIP_TRY(c->out.ensure(back_b));
  HIP_TRY(c->h_out.ensure(back_b));
  for (uint32_t i = 0; i < n_slivers; ++i)
    if (accepted[i])
      std::memcpy(static_cast<uint8_t*>(c->h_in.p) + off[i], slivers[i], sliver_len[i]);
  if (in_b) HIP_TRY(hipMemcpyAsync(c->input.p, c->h_in.p, in_b, hipMemcpyHostToDevice, st));
  uint8_t* dout = c->out.as<uint8_t>();
  const uint8_t* din = c->input.as<uint8_t>();
  RS2_TRY(checker_run(c, plan, [&](uint32_t i) { return din + off[i]; }, expected_roots, dout,
                      expected_roots ? reinterpret_cast<int32_t*>(dout + roots_b) : nullptr, st));
  HIP_TRY(hipMemcpyAsync(c->h_out.p, dout, back_b, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint8_t* ho = static_cast<const uint8_t*>(c->h_out.p);
  // root slots of refused slivers are not written
  if (roots_out)
    for (uint32_t i = 0; i < n_slivers; ++i)
      if (accepted[i]) std::memcpy(roots_out + size_t(i) * 32, ho + size_t(i) * 32, 32);
  if (verdict_out) std::memcpy(verdict_out, ho + roots_b, size_t(n_slivers) * 4);
  return RS2_OK;
}

int rs2_set_verify_mixed_budget(uint64_t bytes) {
  g_vm_budget.store(bytes ? bytes : kVerifyMixedBudget, std::memory_order_relaxed);
  return RS2_OK;
}

int rs2_verify_mixed_stats(uint64_t* stats_out) {
  return read_stats(stats_out,
                    {&g_vm_windows, &g_vm_grouped, &g_vm_single, &g_vm_groups, &g_vm_launches});
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// mixed blob encode: blobs that share only n_shards, a symbol size per blob
// ---------------------------------------------------------------------------------------------
// Mixed blob encode state (rs2_blob_encoder_*): bound to n_shards only; every blob of a call has
// its own length and symbol size (the upload relay's queue, controller.rs:177).
struct rs2_blob_encoder {
  Context* ctx = nullptr;
  hipStream_t stream = nullptr;
  uint16_t n = 0;
  // the three stage templates (planned once, again only when the block limit changed), their jobs
  // with the transform tables attached, and their mixing tables on the device
  BlobStages stages;
  bool bound = false;
  DevBuf mix[kBlobStages];
  // a window's scratch: repair-repair quadrants, leaves, pair hashes and ids in slot order (used
  // when the window's blobs are not neighbours in the caller's arrays), the slivers of a
  // metadata-only call; its tables
  DevBuf both, leaves, hashes, ids, int_primary, int_secondary, tables;
  // blobs the group launches cannot take run through these plans, one per symbol size, the
  // least recently used one replaced once kSinglePlans are held
  static constexpr size_t kSinglePlans = 4;
  std::vector<rs2_plan*> singles;
  // host-buffer form: blobs in, slivers and metadata out
  DevBuf h_blobs, h_primary, h_secondary, h_hashes, h_ids;
  Event done;  // as rs2_verifier::done
  ~rs2_blob_encoder() {
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {
constexpr uint64_t kEncodeMixedBudget = uint64_t(4) << 30;
std::atomic<uint64_t> g_em_budget{kEncodeMixedBudget};
std::atomic<uint64_t> g_em_windows{0}, g_em_grouped{0}, g_em_single{0}, g_em_sizes{0},
    g_em_launches{0};
// Eligible blobs of one window: what keeps its job and offset tables (three jobs a blob, three
// offset arrays a size) within a third of the pinned upload ring, so the compute launches of a
// window (RS2_ENCODE_MIXED_WINDOW_LAUNCHES) never depend on how many blobs and sizes it holds.
constexpr uint32_t kMixedWindowBlobs = RS2_ENCODE_MIXED_WINDOW_BLOBS;

// The stage templates, planned once per encoder (again only when the block limit changed): host
// arithmetic only.
int encoder_stages(rs2_blob_encoder* e) {
  if (e->stages.n == e->n && e->stages.block_max == block_max()) return RS2_OK;
  RS2_TRY(plan_blob_stages(e->n, e->stages));
  e->bound = false;
  return RS2_OK;
}

// Freshly planned stages' device side, as checker_bind.
int encoder_bind(rs2_blob_encoder* e, hipStream_t st) {
  if (e->bound || !e->stages.batchable) return RS2_OK;
  for (int g = 0; g < kBlobStages; ++g) {
    BlobStageCode& code = e->stages.stage[g];
    const PlannedJob& t = code.tmpl;
    CodecJobBatch& j = code.job;
    for (int b = 0; b < j.n_in; ++b) {
      j.in[b].sd_tab = e->ctx->stream(t.C, t.in_sd[size_t(b)], t.ppw);
      if (!j.in[b].sd_tab) return fail(RS2_E_DEVICE, "table upload failed");
      j.in[b].zero_first = group0_zero(t.C, t.in_sd[size_t(b)], t.ppw);
    }
    for (int o = 0; o < j.n_out; ++o) {
      j.out[o].sd_tab = e->ctx->stream(t.C, t.out_sd[size_t(o)], t.ppw);
      if (!j.out[o].sd_tab) return fail(RS2_E_DEVICE, "table upload failed");
      j.out[o].zero_first = group0_zero(t.C, t.out_sd[size_t(o)], t.ppw);
    }
    j.mix_tab = nullptr;
    if (!code.mix.empty()) {
      HIP_TRY(e->mix[g].ensure(code.mix.size() * 2));
      RS2_TRY(upload_pieces(e->ctx, e->mix[g].p, code.mix.data(), code.mix.size() * 2, st));
      j.mix_tab = e->mix[g].as<uint16_t>();
    }
  }
  e->bound = true;
  return RS2_OK;
}

// Where a window's tables lie in the encoder's table buffer (every part 16-byte aligned).
struct BlobTables {
  size_t stage = 0, leaves = 0, jobs = 0, tiles[kBlobStages] = {0, 0, 0}, offs = 0, lens = 0,
         dst_index = 0, bytes = 0;
  size_t class_offs = 0;  // position and copy offsets (int64) of one size class, all stages
};
BlobTables blob_tables(const rs2_blob_encoder* e, const BlobWindow& w) {
  BlobTables t;
  size_t at = 0;
  auto take = [&](size_t n) {
    const size_t here = at;
    at += (n + 15) / 16 * 16;
    return here;
  };
  const size_t ne = w.n_eligible;
  t.stage = take((ne + 1) * sizeof(BlobStage));
  t.leaves = take((ne + 1) * sizeof(BlobLeaves));
  t.jobs = take(kBlobStages * ne * sizeof(CodecJobBatch));
  for (int g = 0; g < kBlobStages; ++g) {
    t.tiles[g] = take(w.tiles[g].size() * 4);
    t.class_offs += e->stages.stage[g].tmpl.offs.size();
  }
  t.offs = take(w.sizes.size() * t.class_offs * 8);
  t.lens = take(ne * 8);
  t.dst_index = take(ne * 4);
  t.bytes = std::max<size_t>(at, 16);
  return t;
}

// The plan of the per-blob path for a blob of `len` bytes and symbol size s: the cached one of
// that size re-bound to the length, else a new one in the place of the least recently used.
int encoder_single_plan(rs2_blob_encoder* e, uint16_t s, uint64_t len, rs2_plan** out) {
  auto& ps = e->singles;
  for (size_t i = 0; i < ps.size(); ++i)
    if (ps[i]->s == s) {
      rs2_plan* p = ps[i];
      ps.erase(ps.begin() + long(i));
      ps.push_back(p);
      RS2_TRY(rs2_plan_rebind(p, len));
      *out = p;
      return RS2_OK;
    }
  if (ps.size() >= rs2_blob_encoder::kSinglePlans) {
    rs2_plan_destroy(ps.front());  // waits for its pending work
    ps.erase(ps.begin());
  }
  rs2_plan* p = nullptr;
  RS2_TRY(rs2_plan_create(e->n, len, &p));
  ps.push_back(p);
  *out = p;
  return RS2_OK;
}

// Run a planned call on st.  src(b): the device address of the caller's blob b; prim(b) / sec(b):
// where its slivers go (not called when meta_only: the window's scratch takes them); lens,
// d_hashes and d_ids are indexed by the caller's blob.  Every buffer is sized for the call's
// largest window before the first window runs.
template <class SrcF, class PrimF, class SecF>
int encoder_run(rs2_blob_encoder* e, const BlobsMixedPlan& plan, const uint64_t* lens, SrcF src,
                PrimF prim, SecF sec, bool meta_only, uint8_t* d_hashes, uint8_t* d_ids,
                hipStream_t st) {
  Context* ctx = e->ctx;
  const BlobStages& sg = e->stages;
  const int64_t n = e->n, kp = sg.kp, ks = sg.ks;
  // a previous call on another stream still owns the scratch buffers and tables
  HIP_TRY(e->done.wait_on(st));
  uint64_t max_both = 0, max_prim = 0, max_sec = 0;
  uint32_t max_elig = 0;
  size_t max_tab = 0;
  for (const BlobWindow& w : plan.windows) {
    if (!w.n_eligible) continue;
    max_both = std::max(max_both, w.both_bytes);
    max_prim = std::max(max_prim, w.primary_bytes);
    max_sec = std::max(max_sec, w.secondary_bytes);
    max_elig = std::max(max_elig, w.n_eligible);
    max_tab = std::max(max_tab, blob_tables(e, w).bytes);
  }
  if (max_elig) {
    RS2_TRY(encoder_bind(e, st));
    HIP_TRY(e->both.ensure(std::max<uint64_t>(max_both, 16)));
    HIP_TRY(e->leaves.ensure(size_t(max_elig) * size_t(n) * size_t(n) * 32));
    HIP_TRY(e->hashes.ensure(size_t(max_elig) * size_t(n) * 64));
    HIP_TRY(e->ids.ensure(size_t(max_elig) * 32));
    HIP_TRY(e->tables.ensure(max_tab));
    if (meta_only) {
      HIP_TRY(e->int_primary.ensure(std::max<uint64_t>(max_prim, 16)));
      HIP_TRY(e->int_secondary.ensure(std::max<uint64_t>(max_sec, 16)));
    }
  }
  uint8_t* const d_tab = e->tables.as<uint8_t>();
  uint8_t* const both = e->both.as<uint8_t>();
  uint8_t* const leaves = e->leaves.as<uint8_t>();
  const int64_t leaves_b = n * n * 32;
  const uint64_t leaf_tiles = uint64_t((n * ks + 255) / 256 + ((n - ks) * kp + 255) / 256 +
                                       ((n - kp) * (n - ks) + 255) / 256);
  std::vector<uint8_t> h_tab;
  for (const BlobWindow& w : plan.windows) {
    const uint32_t ne = w.n_eligible;
    uint64_t launches = 0;
    if (w.slots.empty()) continue;  // every blob of the call was refused
    if (ne) {
      const BlobTables t = blob_tables(e, w);
      h_tab.assign(t.bytes, 0);
      BlobStage* stage = reinterpret_cast<BlobStage*>(h_tab.data() + t.stage);
      BlobLeaves* lv = reinterpret_cast<BlobLeaves*>(h_tab.data() + t.leaves);
      CodecJobBatch* jobs = reinterpret_cast<CodecJobBatch*>(h_tab.data() + t.jobs);
      int64_t* offs = reinterpret_cast<int64_t*>(h_tab.data() + t.offs);
      const int64_t* d_offs = reinterpret_cast<const int64_t*>(d_tab + t.offs);
      uint64_t* wl = reinterpret_cast<uint64_t*>(h_tab.data() + t.lens);
      uint32_t* dst_index = reinterpret_cast<uint32_t*>(h_tab.data() + t.dst_index);
      // the scaled offset arrays, shared by the blobs of one size
      for (size_t c = 0; c < w.sizes.size(); ++c) {
        int64_t* o = offs + c * t.class_offs;
        for (int g = 0; g < kBlobStages; ++g) {
          const std::vector<int64_t>& to = sg.stage[g].tmpl.offs;
          for (size_t q = 0; q < to.size(); ++q) o[q] = to[q] < 0 ? int64_t(-1) : to[q] * int64_t(w.sizes[c]);
          o += to.size();
        }
      }
      uint64_t chunks = 0;
      bool neighbours = true;
      for (uint32_t q = 0; q < ne; ++q) {
        const BlobSlot& sl = w.slots[q];
        const int64_t s = sl.s;
        uint8_t* const p = meta_only ? e->int_primary.as<uint8_t>() + sl.primary_off : prim(sl.blob);
        uint8_t* const sc = meta_only ? e->int_secondary.as<uint8_t>() + sl.secondary_off : sec(sl.blob);
        uint8_t* const bq = both + sl.both_off;
        const uint64_t msg = uint64_t(kp * ks * s);
        stage[q] = {src(sl.blob), p, sg.sys_fused ? nullptr : sc, lens[sl.blob], msg,
                    uint32_t(chunks), uint32_t(s)};
        chunks += (msg + 4095) / 4096;
        if (chunks > 0x7FFFFFFFu) return fail(RS2_E_UNSUPPORTED, "window exceeds the launch grid");
        lv[q] = {p, sc, bq, leaves + int64_t(q) * leaves_b, uint32_t(s), uint32_t(q * leaf_tiles)};
        wl[q] = lens[sl.blob];
        dst_index[q] = sl.blob;
        neighbours = neighbours && sl.blob == w.slots[0].blob + q;
        size_t off_at = size_t(sl.size_class) * t.class_offs;
        for (int g = 0; g < kBlobStages; ++g) {
          const BlobStageCode& code = sg.stage[g];
          const PlannedJob& tp = code.tmpl;
          CodecJobBatch j = code.job;
          j.symbol_size = int32_t(s);
          j.n_pairs = int32_t((s + 3) / 4);
          j.pairs_span = sl.pairs_span[g];
          j.n_lines = int32_t(code.n_lines);
          const uint8_t* in_base = g == kStageColsRep ? sc + ks * kp * s : p;
          uint8_t* out_base = g == kStageColsSys ? p : g == kStageRows ? sc : bq;
          for (int b = 0; b < j.n_in; ++b) {
            j.in[b].base = in_base;
            j.in[b].line_stride = code.in_ls * s;
            j.in[b].pos_off = d_offs + off_at + tp.in_off(b);
            if (g == kStageColsSys && sg.sys_fused) {
              j.in[b].copy_base = sc;
              j.in[b].copy_off = d_offs + off_at + code.n_off + size_t(b) * tp.C;
              j.in[b].copy_line_stride = code.copy_ls * s;
              j.in[b].copy_limit = code.copy_extent * s;
            }
          }
          for (int o = 0; o < j.n_out; ++o) {
            j.out[o].base = out_base;
            j.out[o].line_stride = code.out_ls * s;
            j.out[o].pos_off = d_offs + off_at + tp.out_off(o);
            j.out[o].limit = code.out_extent * s;
          }
          jobs[size_t(g) * ne + q] = j;
          off_at += tp.offs.size();
        }
      }
      stage[ne].chunk0 = uint32_t(chunks);
      lv[ne].first_tile = uint32_t(ne * leaf_tiles);
      if (ne * leaf_tiles > 0x7FFFFFFFu) return fail(RS2_E_UNSUPPORTED, "window exceeds the launch grid");
      for (int g = 0; g < kBlobStages; ++g)
        std::memcpy(h_tab.data() + t.tiles[g], w.tiles[g].data(), w.tiles[g].size() * 4);
      RS2_TRY(upload_pieces(ctx, d_tab, h_tab.data(), t.bytes, st));
      HIP_TRY(rs2k_launch_blob_stage(reinterpret_cast<const BlobStage*>(d_tab + t.stage), int(ne),
                                     int64_t(chunks), int(kp), int(ks), st));
      for (int g = 0; g < kBlobStages; ++g) {
        const PlannedJob& tp = sg.stage[g].tmpl;
        HIP_TRY(launch_encode_groups(
            tp.C, reinterpret_cast<const CodecJobBatch*>(d_tab + t.jobs) + size_t(g) * ne,
            reinterpret_cast<const uint32_t*>(d_tab + t.tiles[g]), int(ne), int(w.tiles[g].back()),
            tp.n_z, tp.mode, st));
      }
      HIP_TRY(rs2k_launch_leaf_hash_blobs(reinterpret_cast<const BlobLeaves*>(d_tab + t.leaves),
                                          int(ne), int64_t(ne * leaf_tiles), int(n), int(kp),
                                          int(ks), st));
      // blobs that are neighbours in the caller's arrays get their hashes and ids in place
      uint8_t* const wh = neighbours ? d_hashes + size_t(w.slots[0].blob) * size_t(n) * 64
                                     : e->hashes.as<uint8_t>();
      uint8_t* const wi = neighbours ? d_ids + size_t(w.slots[0].blob) * 32 : e->ids.as<uint8_t>();
      HIP_TRY(rs2k_launch_merkle_trees(leaves, int(n), int(n), int(n), n * 32, 32, 32, n * 32, wh,
                                       64, st, nullptr, 0, int(ne), leaves_b, n * 64));
      HIP_TRY(rs2k_launch_merkle_root(wh, int(n), 0, wi, st, int(ne),
                                      reinterpret_cast<const uint64_t*>(d_tab + t.lens)));
      launches = 7;
      if (!neighbours) {
        HIP_TRY(rs2k_launch_blob_meta_scatter(
            wh, wi, reinterpret_cast<const uint32_t*>(d_tab + t.dst_index), int(ne), int(n),
            d_hashes, d_ids, st));
        ++launches;
      }
    }
    // the other blobs: the single-blob encode on the same stream, a blob at a time
    for (size_t q = ne; q < w.slots.size(); ++q) {
      const BlobSlot& sl = w.slots[q];
      rs2_plan* p = nullptr;
      RS2_TRY(encoder_single_plan(e, uint16_t(sl.s), lens[sl.blob], &p));
      uint8_t* const bh = d_hashes + size_t(sl.blob) * size_t(n) * 64;
      uint8_t* const bi = d_ids + size_t(sl.blob) * 32;
      if (meta_only)
        RS2_TRY(encode_metadata(p, src(sl.blob), bh, bi, st));
      else
        RS2_TRY(encode_device(p, src(sl.blob), prim(sl.blob), sec(sl.blob), bh, bi, st, true));
    }
    g_em_windows.fetch_add(1, std::memory_order_relaxed);
    g_em_grouped.fetch_add(ne, std::memory_order_relaxed);
    g_em_single.fetch_add(w.slots.size() - ne, std::memory_order_relaxed);
    g_em_sizes.fetch_add(w.sizes.size(), std::memory_order_relaxed);
    g_em_launches.fetch_add(launches, std::memory_order_relaxed);
  }
  HIP_TRY(e->done.record(st));
  return RS2_OK;
}
}  // namespace

extern "C" {

int rs2_blob_encoder_create(uint16_t n_shards, rs2_blob_encoder** out) {
  if (!out) return fail(RS2_E_INVALID_ARGUMENT, "null encoder pointer");
  *out = nullptr;
  uint16_t kp, ks;
  RS2_TRY(rs2_source_symbols_for_n_shards(n_shards, &kp, &ks));
  if (n_shards > kMaxShards) return fail(RS2_E_UNSUPPORTED, "n_shards above 65535");
  Context* ctx = nullptr;
  RS2_TRY(get_context(&ctx));
  auto e = std::make_unique<rs2_blob_encoder>();
  e->ctx = ctx;
  e->n = n_shards;
  HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  *out = e.release();
  return RS2_OK;
}

void rs2_blob_encoder_destroy(rs2_blob_encoder* e) {
  if (!e) return;
  (void)hipSetDevice(e->ctx->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  (void)e->done.sync();  // work queued on a caller's stream
  for (rs2_plan* p : e->singles) rs2_plan_destroy(p);
  const Quiesced quiesced;
  delete e;
}

int rs2_blob_encoder_encode_device_async(
    rs2_blob_encoder* e, uint32_t n_blobs, const uint64_t* blob_lens, const void* d_blobs_base,
    const uint64_t* blob_off, void* d_primary_base, const uint64_t* primary_off,
    void* d_secondary_base, const uint64_t* secondary_off, void* d_hashes, void* d_blob_ids,
    int* status_out, void* stream) {
  if (!e) return fail(RS2_E_INVALID_ARGUMENT, "null encoder");
  if ((d_primary_base == nullptr) != (d_secondary_base == nullptr))
    return fail(RS2_E_INVALID_ARGUMENT, "d_primary_base and d_secondary_base go together");
  const bool meta_only = !d_primary_base;
  bool empty;
  RS2_TRY(batch_count(n_blobs, "blobs in a call",
                      blob_lens && d_blobs_base && blob_off && d_hashes && d_blob_ids &&
                          (meta_only || (primary_off && secondary_off)),
                      &empty));
  if (empty) return RS2_OK;
  RS2_TRY(check_encode_ptrs(d_blobs_base, d_primary_base, d_secondary_base, d_hashes, d_blob_ids));
  HIP_TRY(hipSetDevice(e->ctx->device));
  hipStream_t st = abi_stream(stream, e->stream);
  // every blob is validated, and the call planned, before anything is enqueued
  RS2_TRY(encoder_stages(e));
  BlobsMixedPlan plan;
  RS2_TRY(plan_blobs_mixed(e->stages, n_blobs, blob_lens, blob_off, meta_only ? nullptr : primary_off,
                           meta_only ? nullptr : secondary_off, nullptr, meta_only,
                           g_em_budget.load(std::memory_order_relaxed), kMixedWindowBlobs,
                           status_out, plan));
  const uint8_t* bb = reinterpret_cast<const uint8_t*>(d_blobs_base);
  uint8_t* pb = reinterpret_cast<uint8_t*>(d_primary_base);
  uint8_t* sb = reinterpret_cast<uint8_t*>(d_secondary_base);
  return encoder_run(
      e, plan, blob_lens, [&](uint32_t b) { return bb + blob_off[b]; },
      [&](uint32_t b) { return pb + primary_off[b]; },
      [&](uint32_t b) { return sb + secondary_off[b]; }, meta_only,
      reinterpret_cast<uint8_t*>(d_hashes), reinterpret_cast<uint8_t*>(d_blob_ids), st);
}

int rs2_encode_blobs_with_metadata(uint16_t n_shards, uint32_t n_blobs, const uint8_t* const* blobs,
                                   const uint64_t* blob_lens, uint8_t* const* primary_out,
                                   uint8_t* const* secondary_out, uint8_t* hashes_out,
                                   uint8_t* blob_ids_out, int* status_out) {
  bool empty;
  RS2_TRY(batch_count(n_blobs, "blobs in a call", blobs && blob_lens, &empty));
  if (empty) return RS2_OK;
  rs2_blob_encoder* enc = nullptr;
  RS2_TRY(rs2_blob_encoder_create(n_shards, &enc));
  std::unique_ptr<rs2_blob_encoder, void (*)(rs2_blob_encoder*)> hold(enc, rs2_blob_encoder_destroy);
  rs2_blob_encoder* e = enc;
  Context* ctx = e->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = e->stream;
  RS2_TRY(encoder_stages(e));
  const bool meta_only = !primary_out && !secondary_out;
  BlobsMixedPlan plan;
  RS2_TRY(plan_blobs_mixed(e->stages, n_blobs, blob_lens, nullptr, nullptr, nullptr, blobs,
                           meta_only, g_em_budget.load(std::memory_order_relaxed),
                           kMixedWindowBlobs, status_out, plan));
  const int64_t n = n_shards, kp = e->stages.kp, ks = e->stages.ks;
  // the accepted blobs and their slivers back to back on the device (256-byte steps)
  std::vector<uint8_t> accepted(n_blobs, 0);
  std::vector<uint32_t> sym(n_blobs, 0);
  for (const BlobWindow& w : plan.windows)
    for (const BlobSlot& sl : w.slots) {
      accepted[sl.blob] = 1;
      sym[sl.blob] = sl.s;
    }
  std::vector<uint64_t> boff(n_blobs, 0), poff(n_blobs, 0), soff(n_blobs, 0);
  uint64_t in_b = 0, p_b = 0, s_b = 0;
  auto step = [](uint64_t v) { return (v + 255) / 256 * 256; };
  for (uint32_t b = 0; b < n_blobs; ++b) {
    if (!accepted[b]) continue;
    boff[b] = in_b;
    in_b += step(std::max<uint64_t>(blob_lens[b], 1));
    if (meta_only) continue;
    poff[b] = p_b;
    soff[b] = s_b;
    p_b += step(uint64_t(n * ks) * sym[b]);
    s_b += step(uint64_t(n * kp) * sym[b]);
  }
  HIP_TRY(e->h_blobs.ensure(std::max<uint64_t>(in_b, 16)));
  HIP_TRY(e->h_hashes.ensure(size_t(n_blobs) * size_t(n) * 64));
  HIP_TRY(e->h_ids.ensure(size_t(n_blobs) * 32));
  if (!meta_only) {
    HIP_TRY(e->h_primary.ensure(std::max<uint64_t>(p_b, 16)));
    HIP_TRY(e->h_secondary.ensure(std::max<uint64_t>(s_b, 16)));
  }
  uint8_t* const db = e->h_blobs.as<uint8_t>();
  uint8_t* const dp = e->h_primary.as<uint8_t>();
  uint8_t* const ds = e->h_secondary.as<uint8_t>();
  uint8_t* const dh = e->h_hashes.as<uint8_t>();
  uint8_t* const di = e->h_ids.as<uint8_t>();
  StagerLease lease(ctx->device);
  struct Drain {  // the ring's slot events were recorded on this encoder's stream (RingGuard)
    Stager* sg;
    Context* ctx;
    ~Drain() {
      for (Event& ev : sg->ev)
        if (ev.set()) {
          (void)ev.sync();
          (void)ev.record(ctx->util_stream);
        }
    }
  } drain{lease.st.get(), ctx};
  std::vector<Seg> segs;
  for (uint32_t b = 0; b < n_blobs; ++b)
    if (accepted[b] && blob_lens[b])
      segs.push_back({const_cast<uint8_t*>(blobs[b]), db + boff[b], size_t(blob_lens[b])});
  RS2_TRY(stage_h2d(ctx, *lease.st, segs, st));
  RS2_TRY(encoder_run(
      e, plan, blob_lens, [&](uint32_t b) { return static_cast<const uint8_t*>(db + boff[b]); },
      [&](uint32_t b) { return dp + poff[b]; }, [&](uint32_t b) { return ds + soff[b]; }, meta_only,
      dh, di, st));
  segs.clear();
  for (uint32_t b = 0; b < n_blobs; ++b) {
    if (!accepted[b]) continue;  // output slots of refused blobs are not written
    const size_t pl = size_t(ks) * sym[b], sl = size_t(kp) * sym[b];
    for (int64_t i = 0; i < n; ++i) {
      if (primary_out && primary_out[size_t(b) * n + i])
        segs.push_back({primary_out[size_t(b) * n + i], dp + poff[b] + size_t(i) * pl, pl});
      if (secondary_out && secondary_out[size_t(b) * n + i])
        segs.push_back({secondary_out[size_t(b) * n + i], ds + soff[b] + size_t(i) * sl, sl});
    }
    if (hashes_out)
      segs.push_back({hashes_out + size_t(b) * n * 64, dh + size_t(b) * n * 64, size_t(n) * 64});
    if (blob_ids_out) segs.push_back({blob_ids_out + size_t(b) * 32, di + size_t(b) * 32, 32});
  }
  if (!segs.empty()) RS2_TRY(stage_d2h(ctx, *lease.st, segs, st));
  HIP_TRY(hipStreamSynchronize(st));
  return RS2_OK;
}

int rs2_set_encode_mixed_budget(uint64_t bytes) {
  g_em_budget.store(bytes ? bytes : kEncodeMixedBudget, std::memory_order_relaxed);
  return RS2_OK;
}

int rs2_encode_mixed_stats(uint64_t* stats_out) {
  return read_stats(stats_out,
                    {&g_em_windows, &g_em_grouped, &g_em_single, &g_em_sizes, &g_em_launches});
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// mixed sliver recovery: slivers that share only n_shards, each recovered from its own received
// symbols, with its own axis and symbol size; and the proof check of such received symbols
// ---------------------------------------------------------------------------------------------
namespace {
std::atomic<uint64_t> g_rm_windows{0}, g_rm_launches{0}, g_rm_batched{0}, g_rm_single{0},
    g_rm_groups{0};

// What a mixed recovery call reads and writes: sliver i's received symbols back to back at
// d_symbols + symbols_off[i], its output at d_out + sliver_off[i].
struct MixedRecoverIo {
  const uint8_t* axis;
  const uint16_t* symbol_size;
  const uint8_t* d_symbols;
  const uint64_t* symbols_off;
  uint8_t* d_out;
  const uint64_t* sliver_off;
};

// Decode window w's accepted slivers (items from next_item on, in the caller's order) on st:
// every sliver is planned on the host pool; the batch-eligible ones leave in range launches, one
// per chunk of cut_range_chunks; the others through the per-sliver decode on the same stream.
int recover_mixed_window(rs2_sliver_checker* c, const SliverWindow& w,
                         const std::vector<MixedRecoverItem>& items, size_t& next_item,
                         const MixedRecoverIo& io, hipStream_t st) {
  Context* ctx = c->ctx;
  const size_t i0 = next_item;
  while (next_item < items.size() && items[next_item].slot < w.first + w.count) ++next_item;
  const size_t cnt = next_item - i0;
  std::vector<BatchBlob> jobs(cnt);
  std::vector<DecodeSpec> specs(cnt);
  pool_for_each(ctx->pool, cnt, [&](size_t i) {
    const MixedRecoverItem& it = items[i0 + i];
    DecodeSpec& sp = specs[i];
    sliver_recover_spec(c->codes[io.axis[it.slot]].k, c->n, int(io.symbol_size[it.slot]), it.chosen,
                        io.d_symbols + io.symbols_off[it.slot], io.d_out + io.sliver_off[it.slot],
                        decode_may_fuse(), sp);
    uint32_t originals = 0;
    for (uint32_t q = 0; q < sp.K; ++q) originals += sp.present[q] >= 0;
    if (originals < sp.K) plan_batch_spec(sp, originals, jobs[i]);
  });
  std::vector<ChunkJob> geo(cnt);
  for (size_t i = 0; i < cnt; ++i)
    geo[i] = {jobs[i].eligible, jobs[i].C, jobs[i].job.pairs_span, jobs[i].logs.size()};
  std::vector<RangeChunk> chunks;
  std::vector<uint32_t> demoted;
  cut_range_chunks(geo, 1, kBatchTableBytes, chunks, demoted);
  for (uint32_t i : demoted) jobs[i].eligible = false;
  const BatchRun run{ctx, c->rbatch, c->rbatch_slot, 1, nullptr, "",
                     g_rm_launches, g_rm_batched, g_rm_single};
  std::vector<BatchBlob*> ch;
  for (const RangeChunk& rc : chunks) {
    ch.clear();
    for (uint32_t m : rc.members) ch.push_back(&jobs[m]);
    RS2_TRY(launch_batch_chunk(run, ch, st, &rc.tiles));
    g_rm_launches.fetch_add(1, std::memory_order_relaxed);
    g_rm_batched.fetch_add(ch.size(), std::memory_order_relaxed);
  }
  for (size_t i = 0; i < cnt; ++i) {
    if (jobs[i].eligible) continue;
    RS2_TRY(run_decode(ctx, c->rdec, c->rdec_slot, specs[i], {}, decode_may_fuse(), 1, nullptr, st));
    g_rm_single.fetch_add(1, std::memory_order_relaxed);
  }
  g_rm_windows.fetch_add(1, std::memory_order_relaxed);
  g_rm_groups.fetch_add(w.groups.size(), std::memory_order_relaxed);
  return RS2_OK;
}

// Run a planned mixed recovery on st: per window the decodes, then -- with roots or verdicts
// asked for -- the window's verification from the recovered slivers in place (checker_run).
int recover_mixed_run(rs2_sliver_checker* c, const SliverGroupsPlan& plan,
                      const std::vector<MixedRecoverItem>& items, const MixedRecoverIo& io,
                      const uint8_t* expected, uint8_t* d_roots, int32_t* d_verdict,
                      hipStream_t st) {
  size_t next_item = 0;
  auto decode = [&](const SliverWindow& w) {
    return recover_mixed_window(c, w, items, next_item, io, st);
  };
  if (d_roots || expected)
    return checker_run(
        c, plan, [&](uint32_t i) -> const uint8_t* { return io.d_out + io.sliver_off[i]; }, expected,
        d_roots, d_verdict, st, decode);
  // a previous call on another stream still owns the decode slots
  HIP_TRY(c->done.wait_on(st));
  for (const SliverWindow& w : plan.windows) RS2_TRY(decode(w));
  HIP_TRY(c->done.record(st));
  return RS2_OK;
}

// The whole-call rules both recovery forms share (`arrays`: the form's own needed arrays).
int check_recover_mixed_call(uint32_t n_slivers, bool arrays, const uint32_t* counts,
                             const void* symbol_idx, const void* symbols, const void* expected,
                             const void* verdict, bool* empty) {
  RS2_TRY(check_mixed_call(n_slivers, arrays && counts, expected, verdict, empty));
  if (*empty) return RS2_OK;
  if (std::accumulate(counts, counts + n_slivers, size_t(0)) && (!symbol_idx || !symbols))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  return RS2_OK;
}

int recover_mixed_plan(rs2_sliver_checker* c, uint32_t n_slivers, const uint8_t* axis,
                       const uint16_t* symbol_size, const uint32_t* counts,
                       const uint16_t* symbol_idx, const uint64_t* symbols_off,
                       const uint64_t* sliver_off, int* status_out,
                       std::vector<MixedRecoverItem>& items, SliverGroupsPlan& plan) {
  RS2_TRY(checker_codes(c));
  return plan_recover_mixed(c->codes, n_slivers, axis, symbol_size, counts, symbol_idx, symbols_off,
                            sliver_off, g_vm_budget.load(std::memory_order_relaxed),
                            kMixedWindowGroups, uint32_t(kBatchChunkJobs), status_out, items, plan);
}

// The whole-call rules of the mixed proof check and its per-sliver tables: per[2i] = sliver i's
// first symbol of the concatenated list, per[2i + 1] = its target; *total = symbols of the call.
int check_symbols_mixed_call(uint16_t n, uint32_t n_slivers, const uint16_t* symbol_size,
                             const uint32_t* counts, const uint16_t* target_index,
                             std::vector<uint32_t>& per, uint64_t* total, uint32_t* max_count) {
  per.assign(size_t(n_slivers) * 2, 0);
  *total = 0;
  *max_count = 0;
  for (uint32_t i = 0; i < n_slivers; ++i) {
    if (target_index[i] >= n)  // merkle.rs verify_proof: the leaf index is below n_leaves
      return fail(RS2_E_INVALID_ARGUMENT, "target index too large");
    if (symbol_size[i] == 0 || symbol_size[i] % 2)
      return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "symbol_size must be a multiple of the required alignment");
    per[2 * i] = uint32_t(*total);
    per[2 * i + 1] = target_index[i];
    *total += counts[i];
    *max_count = std::max(*max_count, counts[i]);
    if (*total > 0x7FFFFFFFu) return fail(RS2_E_INVALID_ARGUMENT, "too many symbols in a call");
  }
  return RS2_OK;
}
}  // namespace

extern "C" {

int rs2_sliver_checker_recover_device_async(
    rs2_sliver_checker* c, uint32_t n_slivers, const uint8_t* axis, const uint16_t* symbol_size,
    const uint32_t* counts, const uint16_t* symbol_idx, const void* d_symbols_base,
    const uint64_t* symbols_off, const uint8_t* expected_roots, void* d_slivers_base,
    const uint64_t* sliver_off, void* d_roots, void* d_verdict, int* status_out, void* stream) {
  if (!c) return fail(RS2_E_INVALID_ARGUMENT, "null checker");
  bool empty;
  RS2_TRY(check_recover_mixed_call(
      n_slivers, axis && symbol_size && symbols_off && d_slivers_base && sliver_off, counts,
      symbol_idx, d_symbols_base, expected_roots, d_verdict, &empty));
  if (empty) return RS2_OK;
  RS2_TRY(check_symbol_ptr(d_symbols_base, "d_symbols_base"));
  RS2_TRY(check_symbol_ptr(d_slivers_base, "d_slivers_base"));
  RS2_TRY(check_digest_ptr(d_roots, "d_roots"));
  RS2_TRY(check_digest_ptr(d_verdict, "d_verdict"));
  HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = abi_stream(stream, c->stream);
  // every sliver is validated, and the call planned, before anything is enqueued
  std::vector<MixedRecoverItem> items;
  SliverGroupsPlan plan;
  RS2_TRY(recover_mixed_plan(c, n_slivers, axis, symbol_size, counts, symbol_idx, symbols_off,
                             sliver_off, status_out, items, plan));
  const MixedRecoverIo io{axis, symbol_size, reinterpret_cast<const uint8_t*>(d_symbols_base),
                          symbols_off, reinterpret_cast<uint8_t*>(d_slivers_base), sliver_off};
  return recover_mixed_run(c, plan, items, io, expected_roots, reinterpret_cast<uint8_t*>(d_roots),
                           reinterpret_cast<int32_t*>(d_verdict), st);
}

int rs2_recover_slivers_mixed(uint16_t n_shards, uint32_t n_slivers, const uint8_t* axis,
                              const uint16_t* symbol_size, const uint32_t* counts,
                              const uint16_t* symbol_idx, const uint8_t* const* symbols,
                              const uint8_t* expected_roots, uint8_t* const* slivers_out,
                              uint8_t* roots_out, int32_t* verdict_out, int* status_out) {
  bool empty;
  RS2_TRY(check_recover_mixed_call(n_slivers, axis && symbol_size && slivers_out, counts,
                                   symbol_idx, symbols, expected_roots, verdict_out, &empty));
  if (empty) return RS2_OK;
  CheckerLease lease;
  RS2_TRY(lease.get(n_shards));
  rs2_sliver_checker* c = lease.c;
  HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->stream;
  std::vector<MixedRecoverItem> items;
  SliverGroupsPlan plan;
  RS2_TRY(recover_mixed_plan(c, n_slivers, axis, symbol_size, counts, symbol_idx, nullptr, nullptr,
                             status_out, items, plan));
  // only the chosen symbols go up, K per accepted sliver, back to back; the slivers come back
  // the same way, the roots and verdicts of all slots behind them: one H2D, one D2H
  std::vector<uint64_t> off(n_slivers, 0);
  uint64_t len_b = 0;
  for (MixedRecoverItem& it : items) {
    if (!slivers_out[it.slot]) return fail(RS2_E_INVALID_ARGUMENT, "null output sliver");
    for (const auto& ch : it.chosen)
      if (!symbols[it.first + ch.second]) return fail(RS2_E_INVALID_ARGUMENT, "null symbol");
    off[it.slot] = len_b;
    len_b += uint64_t(it.chosen.size()) * symbol_size[it.slot];
  }
  const size_t roots_at = (size_t(len_b) + 15) / 16 * 16;
  const size_t verdict_at = roots_at + size_t(n_slivers) * 32;
  const size_t back_b = verdict_at + size_t(n_slivers) * 4;
  HIP_TRY(c->input.ensure(std::max<size_t>(size_t(len_b), 16)));
  HIP_TRY(c->h_in.ensure(std::max<size_t>(size_t(len_b), 16)));
  HIP_TRY(c->out.ensure(back_b));
  HIP_TRY(c->h_out.ensure(back_b));
  for (MixedRecoverItem& it : items) {
    const size_t s = symbol_size[it.slot];
    uint8_t* at = static_cast<uint8_t*>(c->h_in.p) + off[it.slot];
    for (size_t q = 0; q < it.chosen.size(); ++q) {
      std::memcpy(at + q * s, symbols[it.first + it.chosen[q].second], s);
      it.chosen[q].second = uint32_t(q);
    }
  }
  if (len_b) HIP_TRY(hipMemcpyAsync(c->input.p, c->h_in.p, len_b, hipMemcpyHostToDevice, st));
  uint8_t* dout = c->out.as<uint8_t>();
  const bool roots = roots_out || expected_roots;
  const MixedRecoverIo io{axis, symbol_size, c->input.as<uint8_t>(), off.data(), dout, off.data()};
  RS2_TRY(recover_mixed_run(c, plan, items, io, expected_roots, roots ? dout + roots_at : nullptr,
                            expected_roots ? reinterpret_cast<int32_t*>(dout + verdict_at) : nullptr,
                            st));
  HIP_TRY(hipMemcpyAsync(c->h_out.p, dout, back_b, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint8_t* ho = static_cast<const uint8_t*>(c->h_out.p);
  // slots of refused slivers are not written, except verdict_out
  for (const MixedRecoverItem& it : items) {
    std::memcpy(slivers_out[it.slot], ho + off[it.slot],
                it.chosen.size() * size_t(symbol_size[it.slot]));
    if (roots_out)
      std::memcpy(roots_out + size_t(it.slot) * 32, ho + roots_at + size_t(it.slot) * 32, 32);
  }
  if (verdict_out) std::memcpy(verdict_out, ho + verdict_at, size_t(n_slivers) * 4);
  return RS2_OK;
}

int rs2_recover_mixed_stats(uint64_t* stats_out) {
  return read_stats(stats_out,
                    {&g_rm_windows, &g_rm_launches, &g_rm_batched, &g_rm_single, &g_rm_groups});
}

int rs2_sliver_checker_check_recovery_symbols_device_async(
    rs2_sliver_checker* c, uint32_t n_slivers, const uint16_t* symbol_size, const uint32_t* counts,
    const uint16_t* target_index, const void* d_symbols_base, const uint64_t* symbols_off,
    const void* d_proofs, const void* d_expected_roots, void* d_ok, void* stream) {
  if (!c) return fail(RS2_E_INVALID_ARGUMENT, "null checker");
  bool empty;
  RS2_TRY(batch_count(n_slivers, "slivers in a call",
                      symbol_size && counts && target_index && symbols_off, &empty));
  if (empty) return RS2_OK;
  const int L = merkle_path_len(c->n);
  std::vector<uint32_t> per;
  uint64_t total;
  uint32_t max_count;
  RS2_TRY(check_symbols_mixed_call(c->n, n_slivers, symbol_size, counts, target_index, per, &total,
                                   &max_count));
  for (uint32_t i = 0; i < n_slivers; ++i)
    RS2_TRY(check_symbol_step(symbols_off[i], "symbols_off[i]"));
  if (total == 0) return RS2_OK;
  if (!d_symbols_base || !d_expected_roots || !d_ok || (L && !d_proofs))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  RS2_TRY(check_symbol_ptr(d_symbols_base, "d_symbols_base"));
  RS2_TRY(check_digest_ptr(d_proofs, "d_proofs"));
  RS2_TRY(check_digest_ptr(d_expected_roots, "d_expected_roots"));
  RS2_TRY(check_digest_ptr(d_ok, "d_ok"));
  HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = abi_stream(stream, c->stream);
  HIP_TRY(c->done.wait_on(st));
  // the proof check's table, then the leaf launch's runs, through one upload
  const size_t runs_at = (per.size() * 4 + 15) / 16 * 16;
  std::vector<uint8_t> h_tab(runs_at + size_t(n_slivers) * sizeof(SymbolRun), 0);
  std::memcpy(h_tab.data(), per.data(), per.size() * 4);
  SymbolRun* runs = reinterpret_cast<SymbolRun*>(h_tab.data() + runs_at);
  for (uint32_t i = 0; i < n_slivers; ++i)
    runs[i] = {reinterpret_cast<const uint8_t*>(d_symbols_base) + symbols_off[i], per[2 * i],
               counts[i], symbol_size[i], 0};
  HIP_TRY(c->sym_digests.ensure(size_t(total) * 32));
  HIP_TRY(c->per_sliver.ensure(h_tab.size()));
  RS2_TRY(upload_pieces(c->ctx, c->per_sliver.p, h_tab.data(), h_tab.size(), st));
  HIP_TRY(rs2k_launch_leaf_hash_runs(
      reinterpret_cast<const SymbolRun*>(c->per_sliver.as<uint8_t>() + runs_at), int(n_slivers),
      max_count, c->sym_digests.as<uint8_t>(), st));
  HIP_TRY(rs2k_launch_recovery_proof_check(
      c->sym_digests.as<uint8_t>(), c->per_sliver.as<uint32_t>(), int(n_slivers), max_count,
      uint32_t(total), reinterpret_cast<const uint8_t*>(d_proofs), L,
      reinterpret_cast<const uint8_t*>(d_expected_roots), reinterpret_cast<uint8_t*>(d_ok), st));
  HIP_TRY(c->done.record(st));
  return RS2_OK;
}

int rs2_check_recovery_symbols_mixed(uint16_t n_shards, uint32_t n_slivers,
                                     const uint16_t* symbol_size, const uint32_t* counts,
                                     const uint16_t* target_index, const uint8_t* const* symbols,
                                     const uint8_t* proofs, const uint8_t* expected_roots,
                                     uint8_t* ok_out) {
  bool empty;
  RS2_TRY(batch_count(n_slivers, "slivers in a call", symbol_size && counts && target_index, &empty));
  if (empty) return RS2_OK;
  CheckerLease lease;
  RS2_TRY(lease.get(n_shards));
  rs2_sliver_checker* c = lease.c;
  const size_t L = size_t(merkle_path_len(n_shards));
  std::vector<uint32_t> per;
  uint64_t total64;
  uint32_t max_count;
  RS2_TRY(check_symbols_mixed_call(n_shards, n_slivers, symbol_size, counts, target_index, per,
                                   &total64, &max_count));
  const size_t total = size_t(total64);
  if (total == 0) return RS2_OK;
  if (!symbols || !expected_roots || !ok_out || (L && !proofs))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  for (size_t j = 0; j < total; ++j)
    if (!symbols[j]) return fail(RS2_E_INVALID_ARGUMENT, "null symbol");
  HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->stream;
  // symbols (a sliver's back to back), proofs and expected roots through one pinned buffer
  std::vector<uint64_t> off(n_slivers, 0);
  size_t sym_b = 0;
  for (uint32_t i = 0; i < n_slivers; ++i) {
    off[i] = sym_b;
    sym_b += size_t(counts[i]) * symbol_size[i];
  }
  const size_t prf_at = (sym_b + 15) / 16 * 16;
  const size_t exp_at = prf_at + total * L * 32, ok_at = exp_at + total * 32;
  const size_t all_b = ok_at + (total + 15) / 16 * 16;
  HIP_TRY(c->input.ensure(all_b));
  HIP_TRY(c->h_in.ensure(ok_at));
  HIP_TRY(c->h_out.ensure(std::max<size_t>(total, 16)));
  uint8_t* hi = static_cast<uint8_t*>(c->h_in.p);
  for (uint32_t i = 0; i < n_slivers; ++i)
    for (uint32_t q = 0; q < counts[i]; ++q)
      std::memcpy(hi + off[i] + size_t(q) * symbol_size[i], symbols[per[2 * i] + q], symbol_size[i]);
  if (L) std::memcpy(hi + prf_at, proofs, total * L * 32);
  std::memcpy(hi + exp_at, expected_roots, total * 32);
  HIP_TRY(hipMemcpyAsync(c->input.p, hi, ok_at, hipMemcpyHostToDevice, st));
  uint8_t* d = c->input.as<uint8_t>();
  RS2_TRY(rs2_sliver_checker_check_recovery_symbols_device_async(
      c, n_slivers, symbol_size, counts, target_index, d, off.data(), d + prf_at, d + exp_at,
      d + ok_at, nullptr));
  HIP_TRY(hipMemcpyAsync(c->h_out.p, d + ok_at, total, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  std::memcpy(ok_out, c->h_out.p, total);
  return RS2_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// mixed recovery symbols: source slivers that share only n_shards, each with its own axis, symbol
// size and list of targets
// ---------------------------------------------------------------------------------------------
namespace {
std::atomic<uint64_t> g_sm_windows{0}, g_sm_expanded{0}, g_sm_built{0}, g_sm_cached{0},
    g_sm_requests{0}, g_sm_launches{0};

// Run a planned mixed recovery-symbol call on st.  src(i): the device address of the caller's
// sliver i; sym(i): where its first symbol goes.  Per window: one table upload (the group tables
// of the slivers to expand, the slot records, the scatter's index and the first chunk of the
// request table), the expansion (gather, encode groups; the other groups through the per-size
// verifier into the same repair buffer), with BUILD the leaves and the trees in slot order, the
// scatter to the caller's order when d_nodes is given, and the requests in chunks.
template <class SrcF, class SymF>
int symbols_mixed_run(rs2_sliver_checker* c, const SymbolsMixedPlan& plan, const uint8_t* axis,
                      const uint16_t* symbol_size, int trees, SrcF src, SymF sym, uint8_t* d_nodes,
                      uint8_t* d_proofs, hipStream_t st) {
  Context* ctx = c->ctx;
  const int64_t n = c->n, nn = int64_t(plan.n_nodes);
  const bool build = trees == RS2_TREES_BUILD;
  if (plan.accepted == 0) return RS2_OK;  // every sliver refused: nothing is enqueued
  // a previous call on another stream still owns the scratch buffers and tables
  HIP_TRY(c->done.wait_on(st));
  RS2_TRY(checker_bind(c, st));
  // a window's tables: mixed_tables' layout for its expanded slivers, then its own parts
  struct Parts {
    MixedTables t;
    size_t sym_slots = 0, scatter = 0, requests = 0, bytes = 0;
    uint64_t other_repair = 0;  // repair bytes of the groups outside the group launches
  };
  auto parts_of = [&](const SymbolsMixedWindow& w) {
    Parts p;
    p.t = mixed_tables(c, w.ex, false);
    size_t at = p.t.bytes;
    auto take = [&](size_t b) {
      const size_t here = at;
      at += (b + 15) / 16 * 16;
      return here;
    };
    p.sym_slots = take(size_t(w.n_slots) * sizeof(SymbolSlot));
    p.scatter = take(size_t(w.ex.n_slots) * 4);
    p.requests = take(size_t(std::min(w.n_requests, kRequestChunk)) * 4);
    p.bytes = std::max<size_t>(at, 16);
    for (size_t g = size_t(w.ex.axis_groups[0]) + w.ex.axis_groups[1]; g < w.ex.groups.size(); ++g)
      p.other_repair += uint64_t(w.ex.groups[g].count) * uint64_t(n - w.ex.groups[g].k) * w.ex.groups[g].s;
    return p;
  };
  uint64_t max_gather = 0, max_repair = 0;
  uint32_t max_ex = 0;
  size_t max_tab = 0;
  for (const SymbolsMixedWindow& w : plan.windows) {
    const Parts p = parts_of(w);
    max_gather = std::max(max_gather, w.ex.gather_bytes);
    max_repair = std::max(max_repair, w.ex.repair_bytes + p.other_repair);
    max_ex = std::max(max_ex, w.ex.n_slots);
    max_tab = std::max(max_tab, p.bytes);
  }
  HIP_TRY(c->gathered.ensure(std::max<uint64_t>(max_gather, 16)));
  HIP_TRY(c->repair.ensure(std::max<uint64_t>(max_repair, 16)));
  if (build) {
    HIP_TRY(c->leaves.ensure(std::max<size_t>(size_t(max_ex) * size_t(n) * 32, 16)));
    HIP_TRY(c->slot_roots.ensure(std::max<size_t>(size_t(max_ex) * 32, 16)));
    HIP_TRY(c->nodes.ensure(std::max<size_t>(size_t(max_ex) * size_t(nn) * 32, 16)));
  }
  HIP_TRY(c->tables.ensure(max_tab));
  uint8_t* const gath = c->gathered.as<uint8_t>();
  uint8_t* const rep = c->repair.as<uint8_t>();
  uint8_t* const d_tab = c->tables.as<uint8_t>();
  uint8_t* const tree_nodes = c->nodes.as<uint8_t>();
  SymbolLevels lv;
  std::copy(plan.level_base, plan.level_base + kSymbolLevels, lv.base);
  std::vector<uint8_t> h_tab;
  for (const SymbolsMixedWindow& w : plan.windows) {
    if (w.n_slots == 0) continue;  // refused slivers only: no work, not counted
    const SliverWindow& ex = w.ex;
    const Parts p = parts_of(w);
    h_tab.assign(p.bytes, 0);
    uint64_t chunks = 0;
    RS2_TRY(pack_group_tables(c, ex, src, p.t, h_tab.data(), d_tab, gath, rep, &chunks));
    const uint32_t ne = ex.axis_groups[0] + ex.axis_groups[1];
    // slot records: expanded slots find their repair symbols in the window's repair buffer
    SymbolSlot* ss = reinterpret_cast<SymbolSlot*>(h_tab.data() + p.sym_slots);
    for (uint32_t sl = 0; sl < w.n_slots; ++sl) {
      const uint32_t i = w.perm[sl];
      ss[sl].sys = src(i);
      ss[sl].rep = nullptr;
      // (BUILD: a slot that is not expanded has no request, hence no tree)
      ss[sl].nodes = !build               ? d_nodes + int64_t(i) * nn * 32
                     : sl < ex.n_slots    ? tree_nodes + int64_t(sl) * nn * 32
                                          : nullptr;
      ss[sl].sym = sym(i);
      ss[sl].first_request = w.slot_request[sl];
      ss[sl].s = symbol_size[i];
      ss[sl].k = uint16_t(c->codes[axis[i]].k);
    }
    uint64_t other_at = ex.repair_bytes;
    std::vector<uint8_t*> other_rep(ex.groups.size(), nullptr);
    for (size_t g = 0; g < ex.groups.size(); ++g) {
      const SliverGroup& gr = ex.groups[g];
      const uint64_t rl = uint64_t(n - gr.k) * gr.s;
      uint8_t* grep = rep + gr.repair_off;
      if (g >= ne) {
        grep = other_rep[g] = rep + other_at;
        other_at += gr.count * rl;
      }
      for (uint32_t q = 0; q < gr.count; ++q) ss[gr.first_slot + q].rep = grep + q * rl;
    }
    const bool scatter = build && d_nodes && ex.n_slots;
    uint32_t* dst_index = reinterpret_cast<uint32_t*>(h_tab.data() + p.scatter);
    for (uint32_t sl = 0; sl < ex.n_slots; ++sl) dst_index[sl] = w.perm[sl];
    const uint32_t chunk0 = std::min(w.n_requests, kRequestChunk);
    std::memcpy(h_tab.data() + p.requests, plan.table.data() + w.first_request, size_t(chunk0) * 4);
    RS2_TRY(upload_pieces(ctx, d_tab, h_tab.data(), p.bytes, st));
    uint64_t launches = 0;
    RS2_TRY(launch_group_expand(c, ex, p.t, d_tab, gath, chunks, st, &launches));
    // the other groups: the per-size verifier on the same stream, from their gathered copies
    rs2_verifier* v = c->single;
    for (size_t g = ne; g < ex.groups.size(); ++g) {
      const SliverGroup& gr = ex.groups[g];
      v->s = uint16_t(gr.s);
      v->k = uint16_t(gr.k);
      v->axis = gr.axis;
      if (n > int64_t(gr.k))
        RS2_TRY(verifier_expand(v, gath + gr.gather_off, other_rep[g], gr.count, st));
      if (build) {
        SymbolMap map{gath + gr.gather_off, other_rep[g], nullptr, int(n), int(gr.count),
                      int(gr.k), int(gr.s)};
        HIP_TRY(rs2k_launch_leaf_hash(map, 4, int64_t(gr.count) * n, 1,
                                      c->leaves.as<uint8_t>() + int64_t(gr.first_slot) * n * 32, st));
      }
    }
    if (ne < ex.groups.size()) RS2_TRY(verifier_mark_done(v, st));
    if (build && ex.n_slots) {
      if (ex.n_eligible_slots) {
        HIP_TRY(rs2k_launch_leaf_hash_groups(
            reinterpret_cast<const SliverLeafGroup*>(d_tab + p.t.groups), int(ne),
            int(ex.n_eligible_slots), int(n), c->leaves.as<uint8_t>(), st));
        ++launches;
      }
      // every expanded slot's tree at once: leaves and trees are uniform over the window
      HIP_TRY(rs2k_launch_merkle_trees(c->leaves.as<uint8_t>(), int(n), int(ex.n_slots), 0, n * 32,
                                       32, 0, 0, c->slot_roots.as<uint8_t>(), 32, st, tree_nodes,
                                       nn * 32));
      if (n <= int64_t(kGroupMaxLeaves)) ++launches;
    }
    if (scatter) {
      HIP_TRY(rs2k_launch_tree_nodes_scatter(tree_nodes,
                                             reinterpret_cast<const uint32_t*>(d_tab + p.scatter),
                                             int(ex.n_slots), nn, d_nodes, st));
      ++launches;
    }
    // (a window whose requests all belong to refused slivers launches nothing)
    for (uint32_t c0 = 0; w.served && c0 < w.n_requests; c0 += kRequestChunk) {
      const uint32_t cn = std::min(kRequestChunk, w.n_requests - c0);
      const int64_t r0 = int64_t(w.first_request) + c0;
      if (c0)  // the later chunks take the first one's place, in stream order
        RS2_TRY(upload_pieces(ctx, d_tab + p.requests, plan.table.data() + r0, size_t(cn) * 4, st));
      HIP_TRY(rs2k_launch_symbol_requests_slots(
          reinterpret_cast<const SymbolSlot*>(d_tab + p.sym_slots), int(w.n_slots),
          reinterpret_cast<const uint32_t*>(d_tab + p.requests), cn, r0, plan.path_len, lv,
          d_proofs, st));
      ++launches;
    }
    g_sm_windows.fetch_add(1, std::memory_order_relaxed);
    g_sm_expanded.fetch_add(ex.n_slots, std::memory_order_relaxed);
    g_sm_built.fetch_add(build ? ex.n_slots : 0, std::memory_order_relaxed);
    g_sm_cached.fetch_add(build ? 0 : w.with_requests, std::memory_order_relaxed);
    g_sm_requests.fetch_add(w.served, std::memory_order_relaxed);
    g_sm_launches.fetch_add(launches, std::memory_order_relaxed);
  }
  HIP_TRY(c->done.record(st));
  return RS2_OK;
}
}  // namespace

extern "C" {

int rs2_sliver_checker_recovery_symbols_device_async(
    rs2_sliver_checker* c, uint32_t n_slivers, const uint8_t* axis, const uint16_t* symbol_size,
    const void* d_slivers_base, const uint64_t* sliver_off, const uint32_t* target_counts,
    const uint16_t* target_sliver_index, int trees, void* d_nodes, void* d_symbols_base,
    const uint64_t* symbols_off, void* d_proofs, int* status_out, void* stream) {
  if (!c) return fail(RS2_E_INVALID_ARGUMENT, "null checker");
  if (trees != RS2_TREES_BUILD && trees != RS2_TREES_CACHED)
    return fail(RS2_E_INVALID_ARGUMENT, "trees must be RS2_TREES_BUILD or RS2_TREES_CACHED");
  bool empty;
  RS2_TRY(batch_count(n_slivers, "slivers in a call",
                      axis && symbol_size && d_slivers_base && sliver_off && target_counts &&
                          symbols_off,
                      &empty));
  if (empty) return RS2_OK;
  RS2_TRY(check_symbol_ptr(d_slivers_base, "d_slivers_base"));
  RS2_TRY(check_symbol_ptr(d_symbols_base, "d_symbols_base"));
  RS2_TRY(check_digest_ptr(d_proofs, "d_proofs"));
  RS2_TRY(check_digest_ptr(d_nodes, "d_nodes"));
  HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = abi_stream(stream, c->stream);
  // every sliver is validated, and the call planned, before anything is enqueued (a target is
  // remote input on a node)
  RS2_TRY(checker_codes(c));
  SymbolsMixedPlan plan;
  RS2_TRY(plan_symbols_mixed(c->codes, n_slivers, axis, symbol_size, sliver_off, symbols_off,
                             nullptr, nullptr, target_counts, target_sliver_index, trees,
                             d_nodes != nullptr, g_vm_budget.load(std::memory_order_relaxed),
                             kMixedWindowGroups, status_out, plan));
  if (plan.total && (!d_symbols_base || (plan.path_len && !d_proofs)))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  const uint8_t* base = reinterpret_cast<const uint8_t*>(d_slivers_base);
  uint8_t* out = reinterpret_cast<uint8_t*>(d_symbols_base);
  return symbols_mixed_run(
      c, plan, axis, symbol_size, trees, [&](uint32_t i) { return base + sliver_off[i]; },
      [&](uint32_t i) { return out + symbols_off[i]; }, reinterpret_cast<uint8_t*>(d_nodes),
      reinterpret_cast<uint8_t*>(d_proofs), st);
}

int rs2_recovery_symbols_mixed(uint16_t n_shards, uint32_t n_slivers, const uint8_t* axis,
                               const uint16_t* symbol_size, const uint8_t* const* slivers,
                               const uint64_t* sliver_len, const uint32_t* target_counts,
                               const uint16_t* target_sliver_index, uint8_t* const* symbols_out,
                               uint8_t* proofs_out, int* status_out) {
  bool empty;
  RS2_TRY(batch_count(n_slivers, "slivers in a call",
                      axis && symbol_size && slivers && sliver_len && target_counts, &empty));
  if (empty) return RS2_OK;
  CheckerLease lease;
  RS2_TRY(lease.get(n_shards));
  rs2_sliver_checker* c = lease.c;
  HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->stream;
  RS2_TRY(checker_codes(c));
  SymbolsMixedPlan plan;
  RS2_TRY(plan_symbols_mixed(c->codes, n_slivers, axis, symbol_size, nullptr, nullptr, slivers,
                             sliver_len, target_counts, target_sliver_index, RS2_TREES_BUILD, false,
                             g_vm_budget.load(std::memory_order_relaxed), kMixedWindowGroups,
                             status_out, plan));
  // no trees to hand out, or every sliver refused: nothing to do
  if (plan.total == 0 || plan.accepted == 0) return RS2_OK;
  const size_t L = size_t(plan.path_len);
  if (!symbols_out || (L && !proofs_out)) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  // the accepted slivers back to back through pinned staging (one H2D); their symbols come back
  // the same way, the proofs of all requests behind them (one D2H per output range)
  std::vector<uint64_t> in_off(n_slivers, 0), out_off(n_slivers, 0);
  std::vector<uint8_t> accepted(n_slivers, 0);
  for (const SymbolsMixedWindow& w : plan.windows)
    for (uint32_t i : w.perm) accepted[i] = 1;
  uint64_t in_b = 0, sym_b = 0;
  for (uint32_t i = 0; i < n_slivers; ++i) {
    if (!accepted[i]) continue;
    if (target_counts[i] && !symbols_out[i])
      return fail(RS2_E_INVALID_ARGUMENT, "null symbol output");
    in_off[i] = in_b;
    in_b += sliver_len[i];
    out_off[i] = sym_b;
    sym_b += uint64_t(target_counts[i]) * symbol_size[i];
  }
  const size_t prf_at = (size_t(sym_b) + 15) / 16 * 16;
  const size_t prf_b = size_t(plan.total) * L * 32, back_b = prf_at + prf_b;
  HIP_TRY(c->input.ensure(std::max<uint64_t>(in_b, 16)));
  HIP_TRY(c->h_in.ensure(std::max<uint64_t>(in_b, 16)));
  HIP_TRY(c->out.ensure(std::max<size_t>(back_b, 16)));
  HIP_TRY(c->h_out.ensure(std::max<size_t>(back_b, 16)));
  for (uint32_t i = 0; i < n_slivers; ++i)
    if (accepted[i])
      std::memcpy(static_cast<uint8_t*>(c->h_in.p) + in_off[i], slivers[i], sliver_len[i]);
  if (in_b) HIP_TRY(hipMemcpyAsync(c->input.p, c->h_in.p, in_b, hipMemcpyHostToDevice, st));
  const uint8_t* din = c->input.as<uint8_t>();
  uint8_t* dout = c->out.as<uint8_t>();
  RS2_TRY(symbols_mixed_run(
      c, plan, axis, symbol_size, RS2_TREES_BUILD, [&](uint32_t i) { return din + in_off[i]; },
      [&](uint32_t i) { return dout + out_off[i]; }, nullptr, dout + prf_at, st));
  uint8_t* ho = static_cast<uint8_t*>(c->h_out.p);
  if (sym_b) HIP_TRY(hipMemcpyAsync(ho, dout, sym_b, hipMemcpyDeviceToHost, st));
  if (prf_b) HIP_TRY(hipMemcpyAsync(ho + prf_at, dout + prf_at, prf_b, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  // symbol and proof slots of refused slivers are not written
  uint64_t j = 0;
  for (uint32_t i = 0; i < n_slivers; j += target_counts[i], ++i) {
    if (!accepted[i] || !target_counts[i]) continue;
    std::memcpy(symbols_out[i], ho + out_off[i], size_t(target_counts[i]) * symbol_size[i]);
    if (L) std::memcpy(proofs_out + j * L * 32, ho + prf_at + j * L * 32, size_t(target_counts[i]) * L * 32);
  }
  return RS2_OK;
}

int rs2_symbols_mixed_stats(uint64_t* stats_out) {
  return read_stats(stats_out, {&g_sm_windows, &g_sm_expanded, &g_sm_built, &g_sm_cached,
                                &g_sm_requests, &g_sm_launches});
}

int rs2_merkle_root(const uint8_t* leaves, uint32_t n_leaves, uint32_t leaf_len, uint8_t root_out[32]) {
  if ((!leaves && n_leaves) || !root_out) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  if (n_leaves == 0) {  // merkle.rs: an empty tree's root is the all-zero node
    std::memset(root_out, 0, 32);
    return RS2_OK;
  }
  if (leaf_len > 0x7FFFFFFFu / 2) return fail(RS2_E_UNSUPPORTED, "leaf too large");
  Context* ctx = nullptr;
  RS2_TRY(get_context(&ctx));
  hipStream_t st = ctx->util_stream;
  DevBuf din, digests, tmp, root;
  HIP_TRY(din.ensure(size_t(n_leaves) * leaf_len));
  HIP_TRY(digests.ensure(size_t(n_leaves) * 32));
  HIP_TRY(root.ensure(32));
  if (leaf_len)
    HIP_TRY(hipMemcpyAsync(din.p, leaves, size_t(n_leaves) * leaf_len, hipMemcpyHostToDevice, st));
  HIP_TRY(hash_symbols(din.p, n_leaves, int(leaf_len), digests.p, st));
  RS2_TRY(device_merkle_root(digests.as<uint8_t>(), n_leaves, tmp, root.as<uint8_t>(), st));
  HIP_TRY(hipMemcpyAsync(root_out, root.p, 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return RS2_OK;
}

// ---- device 1D codec over strided lines, device hashing primitives -------------------------

int rs2_codec_create(uint16_t k, uint16_t n_shards, uint16_t symbol_size, rs2_codec** out) {
  if (!out) return fail(RS2_E_INVALID_ARGUMENT, "null codec pointer");
  *out = nullptr;
  if (symbol_size == 0 || symbol_size % 2)
    return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "symbol_size must be a multiple of the required alignment");
  if (k == 0 || n_shards <= k) return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "need 0 < k < n_shards");
  if (!rate_supported(k, uint32_t(n_shards) - k))
    return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "unsupported shard count");
  Context* ctx = nullptr;
  RS2_TRY(get_context(&ctx));
  auto c = std::make_unique<rs2_codec>();
  c->ctx = ctx;
  c->n = n_shards;
  c->k = k;
  c->s = symbol_size;
  *out = c.release();
  return RS2_OK;
}

void rs2_codec_destroy(rs2_codec* c) {
  if (!c) return;
  (void)hipSetDevice(c->ctx->device);
  (void)c->enc_done.sync();
  for (auto& sl : c->dec) (void)sl.done.sync();
  const Quiesced quiesced;
  delete c;
}

int rs2_codec_encode_device_async(rs2_codec* c, uint32_t lines, const void* d_src,
                                  uint64_t src_sym_stride, uint64_t src_line_stride,
                                  void* d_repair, uint64_t repair_sym_stride,
                                  uint64_t repair_line_stride, void* stream) {
  if (!c || (lines && (!d_src || !d_repair))) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  RS2_TRY(check_symbol_ptr(d_src, "d_src"));
  RS2_TRY(check_symbol_ptr(d_repair, "d_repair"));
  RS2_TRY(check_codec_step(src_sym_stride, "src_sym_stride"));
  RS2_TRY(check_codec_step(src_line_stride, "src_line_stride"));
  RS2_TRY(check_codec_step(repair_sym_stride, "repair_sym_stride"));
  RS2_TRY(check_codec_step(repair_line_stride, "repair_line_stride"));
  if (lines == 0) return RS2_OK;
  if (src_sym_stride < c->s || repair_sym_stride < c->s)
    return fail(RS2_E_INVALID_ARGUMENT, "symbol stride smaller than the symbol");
  HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t key[4] = {int64_t(src_sym_stride), int64_t(src_line_stride),
                          int64_t(repair_sym_stride), int64_t(repair_line_stride)};
  const uint8_t* src = reinterpret_cast<const uint8_t*>(d_src);
  uint8_t* dst = reinterpret_cast<uint8_t*>(d_repair);
  if (!std::equal(key, key + 4, c->enc_key)) {
    HIP_TRY(c->enc_done.sync());  // old arrays may be in use
    const int64_t ss = key[0], rs = key[2];
    RS2_TRY(plan_encode(uint32_t(c->k), uint32_t(c->n - c->k), int(c->s), src, key[1],
                        [&](uint32_t i) { return int64_t(i) * ss; }, dst, key[3],
                        [&](uint32_t j) { return int64_t(j) * rs; }, INT64_MAX, c->enc));
    RS2_TRY(bind_job(c->ctx, c->enc, c->enc_mem, st));
    std::copy(key, key + 4, c->enc_key);
  }
  for (int b = 0; b < c->enc.job.n_in; ++b) c->enc.job.in[b].base = src;
  for (int o = 0; o < c->enc.job.n_out; ++o) c->enc.job.out[o].base = dst;
  HIP_TRY(launch_job(c->enc, int(lines), st));
  HIP_TRY(c->enc_done.record(st));
  return RS2_OK;
}

int rs2_codec_decode_device_async(rs2_codec* c, uint32_t lines, uint32_t count,
                                  const uint16_t* idx, const void* d_base, const uint64_t* sym_off,
                                  uint64_t line_stride, void* d_out, uint64_t out_sym_stride,
                                  uint64_t out_line_stride, uint64_t out_limit, void* stream) {
  if (!c || (count && (!idx || !sym_off)) || (lines && (!d_base || !d_out)))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  if (out_sym_stride < c->s) return fail(RS2_E_INVALID_ARGUMENT, "symbol stride smaller than the symbol");
  RS2_TRY(check_symbol_ptr(d_base, "d_base"));
  RS2_TRY(check_symbol_ptr(d_out, "d_out"));
  RS2_TRY(check_codec_step(line_stride, "line_stride"));
  RS2_TRY(check_codec_step(out_sym_stride, "out_sym_stride"));
  RS2_TRY(check_codec_step(out_line_stride, "out_line_stride"));
  for (uint32_t i = 0; i < count; ++i) RS2_TRY(check_codec_step(sym_off[i], "sym_off[i]"));
  const int64_t K = c->k, N = c->n, s = c->s;
  // the first K distinct valid indices (the crate ignores duplicates and invalid indices)
  std::vector<int64_t> present(N, -1);
  uint32_t got = 0;
  for (uint32_t i = 0; i < count && got < K; ++i) {
    if (idx[i] >= N || present[idx[i]] >= 0) continue;
    present[idx[i]] = int64_t(sym_off[i]);
    ++got;
  }
  if (got < K) return fail(RS2_E_NOT_ENOUGH_SHARDS, "not enough shards");
  if (lines == 0) return RS2_OK;
  HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  DecodeSpec sp;
  sp.K = uint32_t(K);
  sp.R = uint32_t(N - K);
  sp.symbol_size = int(s);
  sp.present = present;
  sp.src_base = reinterpret_cast<const uint8_t*>(d_base);
  sp.src_ls = int64_t(line_stride);
  sp.dst_base = reinterpret_cast<uint8_t*>(d_out);
  sp.dst_ls = int64_t(out_line_stride);
  sp.dst_limit = int64_t(std::min<uint64_t>(out_limit, uint64_t(INT64_MAX)));
  sp.dst.resize(K);
  for (int64_t i = 0; i < K; ++i) sp.dst[i] = i * int64_t(out_sym_stride);
  // no key: every call plans its erasure pattern anew
  return run_decode(c->ctx, c->dec, c->dec_slot, sp, {}, true, int(lines), nullptr, st);
}

int rs2_copy_segments_device_async(const void* d_src, void* d_dst, uint32_t count_a,
                                   const int64_t* d_src_a, const int64_t* d_dst_a, uint32_t count_b,
                                   int64_t src_b_stride, int64_t dst_b_stride, uint32_t seg_len,
                                   uint32_t unit, void* stream) {
  if (count_a == 0 || count_b == 0 || seg_len == 0) return RS2_OK;
  if (!d_src || !d_dst || !d_src_a || !d_dst_a) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  if (unit != 1 && unit != 2 && unit != 4 && unit != 8 && unit != 16)
    return fail(RS2_E_INVALID_ARGUMENT, "unit must be 1, 2, 4, 8 or 16");
  const auto misaligned = [&](int64_t v) { return v % int64_t(unit) != 0; };
  if (misaligned(int64_t(seg_len)) || misaligned(src_b_stride) || misaligned(dst_b_stride) ||
      misaligned(int64_t(reinterpret_cast<uintptr_t>(d_src))) ||
      misaligned(int64_t(reinterpret_cast<uintptr_t>(d_dst))))
    return fail(RS2_E_INVALID_ARGUMENT, "length, strides or bases not multiples of unit");
  HIP_TRY(rs2k_launch_segment_copy(static_cast<const uint8_t*>(d_src), static_cast<uint8_t*>(d_dst),
                                   count_a, d_src_a, d_dst_a, count_b, src_b_stride, dst_b_stride,
                                   seg_len, int(unit), static_cast<hipStream_t>(stream)));
  return RS2_OK;
}

int rs2_leaf_hashes_device_async(const void* d_symbols, uint64_t count, uint16_t symbol_size,
                                 void* d_leaves, void* stream) {
  if (count && (!d_symbols || !d_leaves)) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  if (symbol_size % 2) return fail(RS2_E_INVALID_ARGUMENT, "symbol_size must be even");
  RS2_TRY(check_symbol_ptr(d_symbols, "d_symbols"));
  RS2_TRY(check_digest_ptr(d_leaves, "d_leaves"));
  if (count == 0) return RS2_OK;
  Context* ctx = nullptr;
  RS2_TRY(get_context(&ctx));
  HIP_TRY(hash_symbols(d_symbols, int64_t(count), int(symbol_size), d_leaves,
                       reinterpret_cast<hipStream_t>(stream)));
  return RS2_OK;
}

int rs2_merkle_roots_device_async(const void* d_leaves, uint32_t n_trees, uint32_t n_leaves,
                                  uint64_t tree_stride, uint64_t leaf_stride, void* d_roots,
                                  uint64_t root_stride, void* stream) {
  if (n_trees && (!d_leaves || !d_roots)) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  if (n_leaves == 0 || n_leaves > uint32_t(kMaxShards))
    return fail(RS2_E_UNSUPPORTED, "trees of 1..65535 leaves supported by this build");
  if (leaf_stride % 16 || tree_stride % 16 || root_stride % 16)
    return fail(RS2_E_INVALID_ARGUMENT, "leaf/tree/root strides must be multiples of 16 bytes");
  RS2_TRY(check_digest_ptr(d_leaves, "d_leaves"));
  RS2_TRY(check_digest_ptr(d_roots, "d_roots"));
  if (n_trees == 0) return RS2_OK;
  Context* ctx = nullptr;
  RS2_TRY(get_context(&ctx));
  // above 4,096 leaves the folded level goes to scratch; the arena quarantines the range when
  // this buffer is released, so the queued launches keep it until the next device sync
  DevBuf scratch;
  if (n_leaves > uint32_t(kMerkleMaxLeaves))
    HIP_TRY(scratch.ensure(tree_scratch_bytes(n_trees, n_leaves)));
  HIP_TRY(rs2k_launch_merkle_trees(reinterpret_cast<const uint8_t*>(d_leaves), int(n_leaves),
                                   int(n_trees), 0, int64_t(tree_stride), int64_t(leaf_stride), 0, 0,
                                   reinterpret_cast<uint8_t*>(d_roots), int64_t(root_stride),
                                   reinterpret_cast<hipStream_t>(stream), nullptr, 0, 1, 0, 0,
                                   scratch.as<uint8_t>()));
  return RS2_OK;
}

int rs2_blob_id_device_async(const void* d_hashes, uint16_t n_shards, uint64_t blob_len,
                             void* d_blob_id, void* stream) {
  if (!d_blob_id || (n_shards && !d_hashes)) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  if (n_shards > kMaxShards) return fail(RS2_E_UNSUPPORTED, "n_shards above 65535");
  RS2_TRY(check_digest_ptr(d_hashes, "d_hashes"));
  RS2_TRY(check_digest_ptr(d_blob_id, "d_blob_id"));
  Context* ctx = nullptr;
  RS2_TRY(get_context(&ctx));
  HIP_TRY(rs2k_launch_merkle_root(reinterpret_cast<const uint8_t*>(d_hashes), n_shards, blob_len,
                                  reinterpret_cast<uint8_t*>(d_blob_id),
                                  reinterpret_cast<hipStream_t>(stream)));
  return RS2_OK;
}

int rs2_blob_id_from_hashes(const uint8_t* hashes, uint16_t n_shards, uint64_t blob_len,
                            uint8_t blob_id_out[32]) {
  if (!hashes || !blob_id_out) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  if (n_shards > kMaxShards) return fail(RS2_E_UNSUPPORTED, "n_shards above 65535");
  Context* ctx = nullptr;
  RS2_TRY(get_context(&ctx));
  hipStream_t st = ctx->util_stream;
  DevBuf dh, bid;
  HIP_TRY(dh.ensure(size_t(n_shards) * 64));
  HIP_TRY(bid.ensure(32));
  if (n_shards)
    HIP_TRY(hipMemcpyAsync(dh.p, hashes, size_t(n_shards) * 64, hipMemcpyHostToDevice, st));
  HIP_TRY(rs2k_launch_merkle_root(dh.as<uint8_t>(), n_shards, blob_len, bid.as<uint8_t>(), st));
  HIP_TRY(hipMemcpyAsync(blob_id_out, bid.p, 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return RS2_OK;
}

int rs2_quilt_layout_device_async(uint16_t n_rows, uint16_t n_cols, uint16_t symbol_size,
                                  const void* d_payload, const int64_t* d_col_off,
                                  const uint32_t* d_col_len, void* d_quilt, void* stream) {
  if (!n_rows || !n_cols || !symbol_size) return fail(RS2_E_INVALID_ARGUMENT, "empty quilt");
  if (symbol_size & 1) return fail(RS2_E_INVALID_ARGUMENT, "symbol size must be even");
  if (!d_payload || !d_col_off || !d_col_len || !d_quilt)
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  Context* ctx = nullptr;
  RS2_TRY(get_context(&ctx));
  HIP_TRY(rs2k_launch_quilt_layout(n_rows, n_cols, symbol_size,
                                   reinterpret_cast<const uint8_t*>(d_payload), d_col_off, d_col_len,
                                   reinterpret_cast<uint8_t*>(d_quilt),
                                   reinterpret_cast<hipStream_t>(stream)));
  return RS2_OK;
}

}  // extern "C"
