// dct_amd/csrc/isolation.hip -- keeping the HIP runtime's rand() use away from the host
// application's rand() stream (RandIsolation, LaunchIsolation: dctq_internal.h).
#include <dlfcn.h>
#include <stdlib.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "dct_amd.h"
#include "dctq_internal.h"

namespace dctq {
namespace {
std::recursive_mutex g_rand_mu;
char g_rand_state[256];  // the runtime's private rand() state, persists across calls
int g_rand_depth = 0;
bool g_rand_init = false;
}  // namespace

RandIsolation::RandIsolation() : saved_(nullptr) {
    g_rand_mu.lock();
    if (g_rand_depth++ == 0) {
        if (!g_rand_init) {
            saved_ = initstate(1u, g_rand_state, sizeof g_rand_state);
            g_rand_init = true;
        } else {
            saved_ = setstate(g_rand_state);
        }
    }
}

RandIsolation::~RandIsolation() {
    if (--g_rand_depth == 0) setstate(saved_);
    g_rand_mu.unlock();
}

namespace {
std::atomic<bool> g_runtime_up{false};  // some entry point initialised the HIP runtime
struct SeenKey {
    int device;
    const void *stream;
    unsigned long long id;  // hipStreamGetId: a re-created stream at a reused handle has another id
    uint64_t entries;       // bit e: entry point e already called by this thread on (device, stream)
};
thread_local std::vector<SeenKey> t_seen;
constexpr unsigned long long kNoId = ~0ull;
}  // namespace

std::atomic<uint32_t> g_grid_limit{0};  // dctq_internal.h limited_grid
thread_local uint32_t t_last_grid = 0;

bool runtime_started() { return g_runtime_up.load(std::memory_order_acquire); }
void note_runtime_started() { g_runtime_up.store(true, std::memory_order_release); }

// The stream's identity: its handle AND its runtime id.  The HIP runtime hands a
// destroyed stream's handle out again to the next hipStreamCreate, so the handle
// alone would take a re-created stream's first call (the one that may create its
// hardware queue, and reach libhsa's rand()) for a steady-state call.
// hipStreamGetId is looked up at run time: a process may have loaded an older HIP
// runtime than the one this library was built against (PyTorch ships its own
// libamdhip64.so.7, without it), and a link-time reference would then keep the
// library from loading.  Without it every stream's id reads 0 (the handle alone;
// hosts then call dctq_stream_release before hipStreamDestroy).
using StreamGetIdFn = hipError_t (*)(hipStream_t, unsigned long long *);
static StreamGetIdFn stream_get_id_fn() {
    static const StreamGetIdFn fn = (StreamGetIdFn)dlsym(RTLD_DEFAULT, "hipStreamGetId");
    return fn;
}
static unsigned long long stream_id(const void *stream) {
    const StreamGetIdFn fn = stream_get_id_fn();
    if (!fn) return 0;
    unsigned long long id = 0;
    if (fn((hipStream_t)stream, &id) != hipSuccess) {  // e.g. a special handle: the handle alone
        (void)hipGetLastError();
        return 0;
    }
    return id;
}

LaunchIsolation::LaunchIsolation(const void *stream, Entry entry) {
    const uint64_t bit = 1ull << entry;
    int dev = -1;
    unsigned long long id = kNoId;
    if (runtime_started() && hipGetDevice(&dev) == hipSuccess) {
        id = stream_id(stream);
        for (const SeenKey &k : t_seen)
            if (k.device == dev && k.stream == stream && k.id == id && (k.entries & bit))
                return;  // steady state: no lock
    }
    iso_.emplace();
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return;  // the call itself reports the error
    note_runtime_started();
    if (id == kNoId) id = stream_id(stream);
    for (SeenKey &k : t_seen)
        if (k.device == dev && k.stream == stream) {
            if (k.id != id) k = SeenKey{dev, stream, id, 0ull};  // the handle now names another stream
            k.entries |= bit;
            return;
        }
    // a host that creates streams without end: forget them all now and then (each stream's
    // next first call is isolated again, which only costs that call the lock)
    if (t_seen.size() >= 64) t_seen.clear();
    t_seen.push_back(SeenKey{dev, stream, id, bit});
}

// dctq_stream_release: this thread forgets the stream (a host about to destroy it).
void forget_stream(const void *stream) {
    for (size_t i = 0; i < t_seen.size();)
        if (t_seen[i].stream == stream) {
            t_seen[i] = t_seen.back();
            t_seen.pop_back();
        } else {
            ++i;
        }
}
}  // namespace dctq

extern "C" {

// The library holds no per-stream memory (the tie-queue kernel and its pixel stash
// are the diagnostic library's, fdct8_diag.hip); the calling thread only forgets
// the stream in its launch-isolation list, so a stream later created at the same
// handle is isolated on its first call even where the runtime cannot tell the two
// apart by id.
int dctq_stream_release(void *stream) {
    dctq::forget_stream(stream);
    return DCTQ_OK;
}

}  // extern "C"
