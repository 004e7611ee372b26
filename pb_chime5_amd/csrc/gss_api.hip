// Context, memory plumbing, profiling and the fused per-utterance pipeline of
// libgss_hip.so (C ABI declared in include/gss_hip.h).
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "gss_internal.h"

// Every entry point that touches the device makes the context's GPU current first:
// one process (and thread) may interleave contexts of different GPUs.
#define GSS_ENTER(ctx)                                   \
    if (!(ctx)) return GSS_ERR_INVALID;                  \
    GSS_HIP_CHECK((ctx), hipSetDevice((ctx)->device))
// entry points whose kernels have GSS_VARIANT switches (WPE, EM, the fused pipeline)
#define GSS_ENTER_VARIANTS(ctx) \
    GSS_ENTER(ctx);             \
    GSS_TRY(variant_refresh(ctx))
static int variant_refresh(gss_ctx *ctx);

// status words [0] and [2] (gss_ctx::status_host; the other words: GSS_STATUS_* in gss_internal.h)
#define GSS_STATUS_REF_CHANNEL 0
#define GSS_STATUS_WPE_ZERO_PIVOTS 2

// ------------------------------------------------------------------ errors
// (gss_host_malloc / gss_host_free are documented as callable from any thread -- the session
// driver's loader threads grow their staging blocks on the first context while its owner
// enqueues: the message of a context is written and read under one lock, and
// gss_last_error() hands out the calling thread's own copy)
static std::mutex g_error_lock;

int gss_fail(gss_ctx *ctx, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) {
        std::lock_guard<std::mutex> guard(g_error_lock);
        ctx->error = buf;
    }
    return code;
}

static thread_local std::string g_create_error;

// ------------------------------------------------------------------ GSS_VARIANT
namespace {
const char *const kVariantKeys[] = {
    // wpe.hip
    "corr_ts", "corr_nw", "corr_blocked", "corr_p_tiles", "chol_diag_unfolded", "apply_ph",
    "apply_generic", "prof_detail", "corr_stg8", "corr_ksplit", "apply_gglobal", "wpe_halves",
    "remainder_full_tile",
    // cacgmm.hip
    "em_wgs", "estep_wpb", "estep_lds", "mstep_prefetch_d", "mstep_tiled", "mstep_plan_min_d",
    "mstep_chunked", "mstep_slots", "force_eigh", "em_unfused", "em_l3_mb", "em_l3_fit_mb",
    "em_streams", "mstep_maxseg", "em4_cold_eigh", "mstep_generic",
    // wpe_online.hip (read by the entry points below)
    "wpe_online_mem"};
struct VariantTable {
    std::mutex lock;
    std::string text;
    bool parsed = false;
    std::map<std::string, int> values;
};
VariantTable &variant_table() {
    static VariantTable t;
    return t;
}
}   // namespace

// Re-read GSS_VARIANT (once per top-level call that launches variant-switched kernels -- the
// kernels' host code below only looks at the parsed table).  An unknown key is an error of that
// call, not an abort() of the host process.  The text may only be changed while no library call
// is in flight: getenv() beside a concurrent setenv() is undefined behaviour in glibc.
static int variant_refresh(gss_ctx *ctx) {
    const char *env = getenv("GSS_VARIANT");
    VariantTable &t = variant_table();
    std::lock_guard<std::mutex> guard(t.lock);
    if (t.parsed && t.text == (env ? env : "")) return GSS_OK;
    t.text = env ? env : "";
    t.parsed = true;
    t.values.clear();
    std::string unknown;
    size_t pos = 0;
    while (pos < t.text.size()) {
        size_t end = t.text.find_first_of(", ", pos);
        if (end == std::string::npos) end = t.text.size();
        const std::string tok = t.text.substr(pos, end - pos);
        pos = end + 1;
        if (tok.empty()) continue;
        const size_t eq = tok.find('=');
        const std::string name = tok.substr(0, eq);
        bool known = false;
        for (const char *k : kVariantKeys) known = known || name == k;
        if (!known) {
            unknown = name;
            continue;
        }
        t.values[name] = eq == std::string::npos ? 1 : atoi(tok.c_str() + eq + 1);
    }
    if (!unknown.empty()) {
        t.values.clear();
        t.parsed = false;       // the next call reports it again
        return gss_fail(ctx, GSS_ERR_INVALID, "GSS_VARIANT names no switch '%s'", unknown.c_str());
    }
    return GSS_OK;
}

int gss_variant(const char *key, int dflt) {
    VariantTable &t = variant_table();
    std::lock_guard<std::mutex> guard(t.lock);
    const auto it = t.values.find(key);
    return it == t.values.end() ? dflt : it->second;
}

extern "C" const char *gss_last_error(gss_ctx *ctx) {
    if (!ctx) return g_create_error.c_str();
    static thread_local std::string copy;
    std::lock_guard<std::mutex> guard(g_error_lock);
    copy = ctx->error;
    return copy.c_str();
}

extern "C" const char *gss_version(void) {
#ifdef GSS_EXPERIMENT_BUILD
    return "pb_chime5_amd/libgss_hip 0.4 EXPERIMENT BUILD (gfx950, f64)";
#else
    return "pb_chime5_amd/libgss_hip 0.4 (gfx950, f64)";
#endif
}

extern "C" int gss_abi_version(void) { return GSS_ABI_VERSION; }

// ------------------------------------------------------------------ context
extern "C" int gss_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count;
}

extern "C" int gss_device_pci_bus_id(int device_id, char *buf, int len) {
    if (!buf || len < 16) return GSS_ERR_INVALID;
    buf[0] = 0;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device_id < 0 || device_id >= count)
        return GSS_ERR_INVALID;
    return hipDeviceGetPCIBusId(buf, len, device_id) == hipSuccess ? GSS_OK : GSS_ERR_HIP;
}

extern "C" int gss_create(int device_id, gss_ctx **out) {
    if (!out) return GSS_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) {
        g_create_error = "no HIP device available: ";
        g_create_error += hipGetErrorString(e);
        return GSS_ERR_HIP;
    }
    if (device_id < 0 || device_id >= count) {
        g_create_error = "device_id out of range";
        return GSS_ERR_INVALID;
    }
    e = hipSetDevice(device_id);
    if (e != hipSuccess) {
        g_create_error = hipGetErrorString(e);
        return GSS_ERR_HIP;
    }
    gss_ctx *ctx = new gss_ctx();
    ctx->device = device_id;
    e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        g_create_error = hipGetErrorString(e);
        delete ctx;
        return GSS_ERR_HIP;
    }
    ctx->stream = ctx->own_stream;
    e = hipHostMalloc(reinterpret_cast<void **>(&ctx->status_host), GSS_STATUS_BYTES,
                      hipHostMallocMapped);
    if (e == hipSuccess)
        e = hipHostGetDevicePointer(reinterpret_cast<void **>(&ctx->status_dev), ctx->status_host, 0);
    if (e != hipSuccess) {
        g_create_error = hipGetErrorString(e);
        (void)hipStreamDestroy(ctx->own_stream);
        delete ctx;
        return GSS_ERR_HIP;
    }
    ctx->status_host[GSS_STATUS_REF_CHANNEL] = INT32_MIN;
    ctx->status_host[GSS_STATUS_WPE_ZERO_PIVOTS] = 0;
    ctx->status_host[GSS_STATUS_SEGMENT_FALLBACKS] = 0;
    ctx->status_host[GSS_STATUS_LCMV_INTERFERER] = -1;
    ctx->status_host[GSS_STATUS_LCMV_FALLBACKS] = 0;
    ctx->status_host[GSS_STATUS_WPD_ZERO_PIVOTS] = 0;
    ctx->status_host[GSS_STATUS_ALIGN_MOVED] = 0;
    *out = ctx;
    return GSS_OK;
}

static void free_tables(gss_ctx *ctx) {
    if (ctx->win_analysis) (void)hipFree(ctx->win_analysis);
    if (ctx->win_synthesis) (void)hipFree(ctx->win_synthesis);
    if (ctx->twiddle) (void)hipFree(ctx->twiddle);
    ctx->win_analysis = ctx->win_synthesis = nullptr;
    ctx->twiddle = nullptr;
}

extern "C" int gss_destroy(gss_ctx *ctx) {
    if (!ctx) return GSS_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    free_tables(ctx);
    if (ctx->arena) (void)hipFree(ctx->arena);
    if (ctx->wpe_tiles) (void)hipFree(ctx->wpe_tiles);
    if (ctx->status_host) (void)hipHostFree(ctx->status_host);
    for (auto &p : ctx->prof_pending) {
        (void)hipEventDestroy(p.start);
        (void)hipEventDestroy(p.stop);
    }
    for (auto ev : ctx->event_pool) (void)hipEventDestroy(ev);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->aux_stream) {
        (void)hipStreamSynchronize(ctx->aux_stream);
        (void)hipStreamDestroy(ctx->aux_stream);
    }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return GSS_OK;
}

int aux_stream_ready(gss_ctx *ctx) {
    if (!ctx->aux_stream)
        GSS_HIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking));
    if (!ctx->ev_fork) GSS_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    if (!ctx->ev_join) GSS_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
    return GSS_OK;
}

extern "C" int gss_set_stream(gss_ctx *ctx, void *hip_stream) {
    GSS_ENTER(ctx);
    GSS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    return GSS_OK;
}

extern "C" int gss_set_utterances_in_flight(gss_ctx *ctx, int n) {
    if (!ctx) return GSS_ERR_INVALID;
    GSS_REQUIRE(ctx, n >= 0, GSS_ERR_INVALID, "gss_set_utterances_in_flight: n=%d", n);
    ctx->utterances_in_flight = n;
    return GSS_OK;
}

extern "C" int gss_synchronize(gss_ctx *ctx) {
    if (!ctx) return GSS_ERR_INVALID;
    GSS_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    GSS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return GSS_OK;
}

// ------------------------------------------------------------------ memory
extern "C" int gss_dev_malloc(gss_ctx *ctx, size_t bytes, void **dev_ptr) {
    if (!ctx || !dev_ptr) return GSS_ERR_INVALID;
    GSS_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    *dev_ptr = nullptr;
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(dev_ptr, bytes);
    if (e != hipSuccess)
        return gss_fail(ctx, GSS_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes,
                        hipGetErrorString(e));
    if (ctx->debug_pattern >= 0)    // workspace debug mode: outputs and states start poisoned too
        GSS_HIP_CHECK(ctx, hipMemsetAsync(*dev_ptr, ctx->debug_pattern, bytes, ctx->stream));
    return GSS_OK;
}

extern "C" int gss_dev_free(gss_ctx *ctx, void *dev_ptr) {
    if (!ctx) return GSS_ERR_INVALID;
    if (!dev_ptr) return GSS_OK;
    GSS_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    GSS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    GSS_HIP_CHECK(ctx, hipFree(dev_ptr));
    return GSS_OK;
}

extern "C" int gss_memcpy_h2d(gss_ctx *ctx, void *dst, const void *src, size_t bytes) {
    GSS_ENTER(ctx);
    if (bytes == 0) return GSS_OK;
    GSS_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    // pageable host memory: the copy is staged before the call returns, but be
    // explicit so the caller may reuse `src` immediately.
    GSS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return GSS_OK;
}

extern "C" int gss_memcpy_d2h(gss_ctx *ctx, void *dst, const void *src, size_t bytes) {
    GSS_ENTER(ctx);
    if (bytes == 0) return GSS_OK;
    GSS_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    GSS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return GSS_OK;
}

// Page-locked host memory + copies that do not wait: the session driver's staging buffers.
// WAV samples are read straight into a pinned (D, N) int16 block, one DMA brings it to the
// device while the host thread goes on to enqueue the kernels behind it.
extern "C" int gss_host_malloc(gss_ctx *ctx, size_t bytes, void **host_ptr) {
    if (!ctx || !host_ptr) return GSS_ERR_INVALID;
    GSS_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    *host_ptr = nullptr;
    if (bytes == 0) bytes = 16;
    hipError_t e = hipHostMalloc(host_ptr, bytes, hipHostMallocDefault);
    if (e != hipSuccess)
        return gss_fail(ctx, GSS_ERR_NOMEM, "hipHostMalloc(%zu) failed: %s", bytes,
                        hipGetErrorString(e));
    return GSS_OK;
}

extern "C" int gss_host_free(gss_ctx *ctx, void *host_ptr) {
    if (!ctx) return GSS_ERR_INVALID;
    if (!host_ptr) return GSS_OK;
    // no stream synchronisation of our own (unlike gss_dev_free); the caller guarantees that
    // no copy from / to the block is still in flight.  hipHostFree itself waits for the whole
    // device, which is why the session driver only frees at the end of a session
    GSS_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    GSS_HIP_CHECK(ctx, hipHostFree(host_ptr));
    return GSS_OK;
}

extern "C" int gss_memcpy_h2d_async(gss_ctx *ctx, void *dst, const void *src, size_t bytes) {
    GSS_ENTER(ctx);
    if (bytes == 0) return GSS_OK;
    GSS_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return GSS_OK;
}

extern "C" int gss_memcpy_d2h_async(gss_ctx *ctx, void *dst, const void *src, size_t bytes) {
    GSS_ENTER(ctx);
    if (bytes == 0) return GSS_OK;
    GSS_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return GSS_OK;
}

extern "C" int gss_memset(gss_ctx *ctx, void *dst, int value, size_t bytes) {
    GSS_ENTER(ctx);
    if (bytes == 0) return GSS_OK;
    GSS_HIP_CHECK(ctx, hipMemsetAsync(dst, value, bytes, ctx->stream));
    return GSS_OK;
}

// ------------------------------------------------------------------ arena
void arena_reset(gss_ctx *ctx) { ctx->arena_off = 0; }

// ---- workspace debug mode (gss_debug_workspace): plain host code around the arena, off by default
namespace {
constexpr size_t kDebugGuard = 256;             // bytes of pattern behind every block (plus its alignment slack)
constexpr size_t kDebugHeadroom = 1 << 20;      // room for the guards of 2048 blocks per reserve

// the debug mode owns the streams while it looks at memory: the internal second stream is
// forked from and joined to ctx->stream by events, which a host-side check does not see
int debug_sync(gss_ctx *ctx) {
    GSS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->aux_stream) GSS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->aux_stream));
    if (ctx->stream != ctx->own_stream) GSS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->own_stream));
    return GSS_OK;
}

// compares one guard with the pattern (the streams are idle); a violated guard counts once
int debug_check_guard(gss_ctx *ctx, gss_ctx::DebugGuard &g) {
    if (g.reported) return GSS_OK;
    unsigned char host[2 * kDebugGuard];
    GSS_HIP_CHECK(ctx, hipMemcpy(host, ctx->arena + g.guard_off, g.guard_bytes, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < g.guard_bytes; ++i) {
        if (host[i] == (unsigned char)ctx->debug_pattern) continue;
        g.reported = true;
        if (ctx->debug_violations++ == 0) {
            char text[512];
            snprintf(text, sizeof(text),
                     "workspace block %d%s%s (logical offset %zu, %zu bytes): byte %zu behind its "
                     "end holds 0x%02x, the guard pattern is 0x%02x",
                     g.block, g.tag ? " " : "", g.tag ? g.tag : "", g.logical_off, g.bytes, i,
                     (unsigned)host[i], (unsigned)ctx->debug_pattern);
            ctx->debug_first = text;
        }
        break;
    }
    return GSS_OK;
}

int debug_check_live_guards(gss_ctx *ctx) {
    if (ctx->debug_guards.empty()) return GSS_OK;
    GSS_TRY(debug_sync(ctx));
    for (auto &g : ctx->debug_guards) GSS_TRY(debug_check_guard(ctx, g));
    return GSS_OK;
}
}   // namespace

int arena_reserve(gss_ctx *ctx, size_t bytes) {
    bytes = align_up(bytes + 4096, 1 << 20);
    const bool debug = ctx->debug_pattern >= 0;
    if (debug) {
        // the guards of the previous call are looked at one last time; the blocks of this call
        // get room for theirs beyond what the sizing formulas ask for
        GSS_TRY(debug_check_live_guards(ctx));
        ctx->debug_guards.clear();
        ctx->debug_blocks = 0;
        ctx->debug_phys = 0;
        ctx->debug_logical_size = bytes;
        bytes += kDebugHeadroom;
    }
    ctx->arena_off = 0;
    if (bytes > ctx->arena_size) {
        GSS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->arena) {
            GSS_HIP_CHECK(ctx, hipFree(ctx->arena));
            ctx->arena = nullptr;
            ctx->arena_size = 0;
        }
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&ctx->arena), bytes);
        if (e != hipSuccess)
            return gss_fail(ctx, GSS_ERR_NOMEM, "workspace hipMalloc(%zu) failed: %s", bytes,
                            hipGetErrorString(e));
        ctx->arena_size = bytes;
    }
    // (nothing that lived before a reserve survives it: poisoning all of it is always legal)
    if (debug) {
        GSS_TRY(debug_sync(ctx));
        GSS_HIP_CHECK(ctx, hipMemsetAsync(ctx->arena, ctx->debug_pattern, ctx->arena_size, ctx->stream));
    }
    return GSS_OK;
}

void *arena_alloc(gss_ctx *ctx, size_t bytes, const char *tag) {
    size_t off = align_up(ctx->arena_off, 256);
    if (ctx->debug_pattern >= 0) {
        // the same logical bump (and the same "too small" answer) as the plain arena; the block
        // itself goes behind the guard of its predecessor
        // (bounded by what THIS reserve asked for, where the plain arena is bounded by the size
        // it has grown to: a sizing formula that is too small fails here on a warm context too)
        if (off + bytes > ctx->debug_logical_size) return nullptr;
        const size_t phys = align_up(ctx->debug_phys, 256);
        const size_t guard_end = align_up(phys + bytes, 256) + kDebugGuard;
        if (guard_end > ctx->arena_size) {
            // the headroom holds the guards of 2048 live blocks, fifty times what a call has: this
            // is the mode running out, not the call's formula, and the report says so
            if (ctx->debug_violations++ == 0) {
                char text[256];
                snprintf(text, sizeof(text),
                         "the guard headroom of the workspace debug mode (%zu bytes) is used up at "
                         "block %d%s%s: no sizing bug of the call",
                         kDebugHeadroom, ctx->debug_blocks, tag ? " " : "", tag ? tag : "");
                ctx->debug_first = text;
            }
            return nullptr;
        }
        ctx->debug_guards.push_back({ctx->debug_blocks++, off, bytes, phys + bytes,
                                     guard_end - (phys + bytes), tag, false});
        ctx->debug_phys = guard_end;
        ctx->arena_off = off + bytes;
        if (ctx->arena_off > ctx->arena_peak) ctx->arena_peak = ctx->arena_off;
        return ctx->arena + phys;
    }
    if (off + bytes > ctx->arena_size) return nullptr;  // reserve() was too small: bug
    ctx->arena_off = off + bytes;
    if (ctx->arena_off > ctx->arena_peak) ctx->arena_peak = ctx->arena_off;
    return ctx->arena + off;
}

// arena_release with the debug mode on: the guards of the released blocks are checked, then
// everything above the mark is poisoned again -- the next stage starts in the pattern, not in
// its predecessor's numbers.  Synchronises both streams first: the second stream may still own
// blocks above the mark, whatever the events say to the first.
int arena_release_debug(gss_ctx *ctx, size_t mark) {
    GSS_TRY(debug_sync(ctx));
    // released: the blocks that end above the mark.  (An empty block that sits exactly on the
    // mark could have been allocated on either side of it; it stays, nothing lives in it.)
    while (!ctx->debug_guards.empty() &&
           ctx->debug_guards.back().logical_off + ctx->debug_guards.back().bytes > mark) {
        GSS_TRY(debug_check_guard(ctx, ctx->debug_guards.back()));
        ctx->debug_guards.pop_back();
    }
    ctx->arena_off = mark;
    ctx->debug_phys = ctx->debug_guards.empty()
                          ? 0
                          : ctx->debug_guards.back().guard_off + ctx->debug_guards.back().guard_bytes;
    GSS_HIP_CHECK(ctx, hipMemsetAsync(ctx->arena + ctx->debug_phys, ctx->debug_pattern,
                                      ctx->arena_size - ctx->debug_phys, ctx->stream));
    return GSS_OK;
}

extern "C" int gss_debug_workspace(gss_ctx *ctx, int pattern) {
    GSS_ENTER(ctx);
    GSS_REQUIRE(ctx, pattern >= -1 && pattern <= 255, GSS_ERR_INVALID,
                "gss_debug_workspace: pattern=%d (a byte, or -1 for off)", pattern);
    GSS_TRY(debug_sync(ctx));
    // a switch starts a new record; the arena keeps its size (a plain reserve never shrinks it)
    ctx->debug_pattern = pattern;
    ctx->debug_guards.clear();
    ctx->debug_blocks = 0;
    ctx->debug_phys = 0;
    ctx->debug_logical_size = 0;
    ctx->debug_violations = 0;
    ctx->debug_first.clear();
    ctx->arena_off = 0;
    // (the WPE tile tables are rebuilt, into a poisoned block, by the next WPE call)
    ctx->wpe_tiles_key[0] = ctx->wpe_tiles_key[1] = ctx->wpe_tiles_key[2] = ctx->wpe_tiles_key[3] = -1;
    return GSS_OK;
}

extern "C" int gss_debug_workspace_report(gss_ctx *ctx, int64_t *violations, char *buf, int len,
                                          int guard_index, void **guard_dev) {
    GSS_ENTER(ctx);
    if (guard_dev) *guard_dev = nullptr;
    if (violations) *violations = 0;
    if (buf && len > 0) buf[0] = 0;
    GSS_REQUIRE(ctx, ctx->debug_pattern >= 0, GSS_ERR_INVALID,
                "gss_debug_workspace_report: the workspace debug mode is off");
    GSS_TRY(debug_check_live_guards(ctx));
    if (violations) *violations = ctx->debug_violations;
    if (buf && len > 0) snprintf(buf, (size_t)len, "%s", ctx->debug_first.c_str());
    if (guard_dev && guard_index >= 0 && (size_t)guard_index < ctx->debug_guards.size())
        *guard_dev = ctx->arena + ctx->debug_guards[guard_index].guard_off;
    return GSS_OK;
}

extern "C" size_t gss_workspace_bytes(gss_ctx *ctx) { return ctx ? ctx->arena_peak : 0; }

// ------------------------------------------------------------------ profiling
ProfScope::ProfScope(gss_ctx *c, const char *name) : ctx(c), active(c->profiling) {
    if (active && !c->prof_filter.empty() && c->prof_filter != name) active = false;
    if (!active) return;
    e.name = name;
    auto get = [&]() {
        hipEvent_t ev;
        if (!ctx->event_pool.empty()) {
            ev = ctx->event_pool.back();
            ctx->event_pool.pop_back();
        } else {
            (void)hipEventCreate(&ev);
        }
        return ev;
    };
    e.start = get();
    e.stop = get();
    (void)hipEventRecord(e.start, ctx->stream);
}

ProfScope::~ProfScope() {
    if (!active) return;
    (void)hipEventRecord(e.stop, ctx->stream);
    ctx->prof_pending.push_back(e);
}

static void prof_drain(gss_ctx *ctx) {
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &p : ctx->prof_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.start, p.stop) == hipSuccess) {
            auto &acc = ctx->prof_acc[p.name];
            acc.first += 1;
            acc.second += ms;
        }
        ctx->event_pool.push_back(p.start);
        ctx->event_pool.push_back(p.stop);
    }
    ctx->prof_pending.clear();
}

extern "C" int gss_profile_enable(gss_ctx *ctx, int on) {
    if (!ctx) return GSS_ERR_INVALID;
    ctx->profiling = on != 0;
    return GSS_OK;
}

extern "C" int gss_profile_filter(gss_ctx *ctx, const char *kernel) {
    if (!ctx) return GSS_ERR_INVALID;
    ctx->prof_filter = kernel ? kernel : "";
    return GSS_OK;
}

extern "C" int gss_profile_reset(gss_ctx *ctx) {
    if (!ctx) return GSS_ERR_INVALID;
    prof_drain(ctx);
    ctx->prof_acc.clear();
    return GSS_OK;
}

extern "C" int gss_profile_report(gss_ctx *ctx, char *buf, size_t buf_size) {
    if (!ctx || !buf || buf_size < 4) return GSS_ERR_INVALID;
    prof_drain(ctx);
    std::string s = "{";
    bool first = true;
    for (auto &kv : ctx->prof_acc) {
        char item[256];
        snprintf(item, sizeof(item), "%s\"%s\": {\"calls\": %ld, \"ms\": %.6f}",
                 first ? "" : ", ", kv.first.c_str(), kv.second.first, kv.second.second);
        s += item;
        first = false;
    }
    s += "}";
    if (s.size() + 1 > buf_size) return gss_fail(ctx, GSS_ERR_INVALID, "report buffer too small");
    memcpy(buf, s.c_str(), s.size() + 1);
    return GSS_OK;
}

// ------------------------------------------------------------------ geometry
extern "C" int64_t gss_stft_num_frames(int64_t n, int size, int shift, int fading) {
    if (fading) n += 2 * (int64_t)(size - shift);
    if (n < size) return 1;
    return (n - size + shift - 1) / shift + 1;
}

extern "C" int64_t gss_istft_num_samples(int64_t T, int size, int shift, int fading) {
    int64_t n = T * shift + size - shift;
    if (fading) n -= 2 * (int64_t)(size - shift);
    return n < 0 ? 0 : n;
}

extern "C" int64_t gss_samples_to_stft_frames(int64_t samples, int size, int shift,
                                              int fading) {
    if (fading) samples += 2 * (int64_t)(size - shift);
    // ceil((samples - size + shift) / shift), also for negative numerators
    int64_t num = samples - size + shift;
    int64_t q = num / shift;
    if (num % shift != 0 && num > 0) q += 1;
    return q;
}

extern "C" int gss_set_windows(gss_ctx *ctx, int size, int shift, const double *analysis,
                               const double *synthesis) {
    if (!ctx || !analysis || !synthesis) return GSS_ERR_INVALID;
    // (powers of two take the radix-2 kernels, other even lengths a direct DFT)
    GSS_REQUIRE(ctx, size >= 4 && size <= GSS_MAX_STFT_SIZE && size % 2 == 0,
                GSS_ERR_UNSUPPORTED, "stft size %d: need an even length in [4, %d]", size,
                GSS_MAX_STFT_SIZE);
    GSS_REQUIRE(ctx, shift > 0 && shift <= size && size % shift == 0, GSS_ERR_INVALID,
                "stft shift %d must divide size %d", shift, size);
    GSS_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    GSS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    free_tables(ctx);
    size_t wb = sizeof(double) * size;
    GSS_HIP_CHECK(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->win_analysis), wb));
    GSS_HIP_CHECK(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->win_synthesis), wb));
    GSS_HIP_CHECK(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->twiddle),
                                 sizeof(cplx) * (size / 2)));
    std::vector<cplx> tw(size / 2);
    for (int j = 0; j < size / 2; ++j) {
        // exact at the quadrant points, cos/sin of a reduced argument elsewhere
        double a = -2.0 * M_PI * (double)j / (double)size;
        tw[j].x = cos(a);
        tw[j].y = sin(a);
    }
    tw[0].x = 1.0;
    tw[0].y = 0.0;
    if (size % 4 == 0) {
        tw[size / 4].x = 0.0;
        tw[size / 4].y = -1.0;
    }
    GSS_HIP_CHECK(ctx, hipMemcpy(ctx->win_analysis, analysis, wb, hipMemcpyHostToDevice));
    GSS_HIP_CHECK(ctx, hipMemcpy(ctx->win_synthesis, synthesis, wb, hipMemcpyHostToDevice));
    GSS_HIP_CHECK(ctx, hipMemcpy(ctx->twiddle, tw.data(), sizeof(cplx) * (size / 2),
                                 hipMemcpyHostToDevice));
    ctx->stft_size = size;
    ctx->stft_shift = shift;
    return GSS_OK;
}

// ------------------------------------------------------------------ stage wrappers

static int check_windows(gss_ctx *ctx) {
    GSS_REQUIRE(ctx, ctx->stft_size > 0, GSS_ERR_INVALID, "call gss_set_windows() first");
    return GSS_OK;
}

static int check_stft_bins(gss_ctx *ctx, int F, int64_t T, int D) {
    const int64_t bins = (int64_t)F * T * D;
    GSS_REQUIRE(ctx, bins < (1LL << 31), GSS_ERR_UNSUPPORTED,
                "F * T * D = %lld STFT bins: 2^31 or more are not supported (some kernels index "
                "the tensor with 32 bits)", (long long)bins);
    return GSS_OK;
}

// beamforming_wrapper.py:44: assert D < 30
static int check_bf_channels(gss_ctx *ctx, int D) {
    GSS_REQUIRE(ctx, D >= 1 && D < 30, GSS_ERR_INVALID, "assert D < 30 failed: D=%d", D);
    return GSS_OK;
}

// pb_bss CACGMMTrainer.fit: assert K < 20 (-> AssertionError in the reference too)
static int check_class_count(gss_ctx *ctx, int K) {
    GSS_REQUIRE(ctx, K >= 1 && K <= GSS_MAX_CLASSES, GSS_ERR_INVALID,
                "cacgmm: assert 1 <= K < 20 failed: K=%d", K);
    return GSS_OK;
}

static int check_target_index(gss_ctx *ctx, int target, int K) {
    GSS_REQUIRE(ctx, target >= 0 && target < K, GSS_ERR_INVALID,
                "target_index %d outside [0, %d)", target, K);
    return GSS_OK;
}

// The WPE argument rule.  `fixed_schedule` (gss_wpe_weighted, one iteration without a PSD
// context): the message names only what the caller gave.
static int check_wpe_args(gss_ctx *ctx, const char *what, int taps, int delay, int iterations,
                          int psd_context, bool fixed_schedule = false) {
    if (taps >= 1 && delay >= 0 && iterations >= 0 && psd_context >= 0) return GSS_OK;
    if (fixed_schedule)
        return gss_fail(ctx, GSS_ERR_INVALID, "%s: taps=%d delay=%d", what, taps, delay);
    return gss_fail(ctx, GSS_ERR_INVALID, "%s: taps=%d delay=%d iterations=%d psd_context=%d", what,
                    taps, delay, iterations, psd_context);
}

extern "C" int gss_stft(gss_ctx *ctx, const double *x, int D, int64_t N, int fading,
                        gss_cplx *Y) {
    GSS_ENTER(ctx);
    GSS_TRY(check_windows(ctx));
    GSS_REQUIRE(ctx, D >= 1 && N >= 0 && x && Y, GSS_ERR_INVALID, "gss_stft: bad arguments");
    return stft_run(ctx, x, 0, D, N, fading, reinterpret_cast<cplx *>(Y));
}

extern "C" int gss_istft(gss_ctx *ctx, const gss_cplx *X, int64_t T, int fading, double *x) {
    GSS_ENTER(ctx);
    GSS_TRY(check_windows(ctx));
    GSS_REQUIRE(ctx, T >= 1 && X && x, GSS_ERR_INVALID, "gss_istft: bad arguments");
    GSS_TRY(arena_reserve(ctx, stft_workspace_bytes(T, ctx->stft_size)));
    return istft_run(ctx, reinterpret_cast<const cplx *>(X), T, fading, x);
}

extern "C" int gss_activity_time_to_frequency(gss_ctx *ctx, const uint8_t *act, int K,
                                              int64_t N, int fading, uint8_t *out) {
    GSS_ENTER(ctx);
    GSS_TRY(check_windows(ctx));
    GSS_REQUIRE(ctx, K >= 1 && N >= 0 && act && out, GSS_ERR_INVALID,
                "gss_activity_time_to_frequency: bad arguments");
    return activity_run(ctx, act, K, N, fading, out);
}

extern "C" int gss_wpe(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D, int taps,
                       int delay, int iterations, int psd_context, gss_cplx *X) {
    GSS_ENTER_VARIANTS(ctx);
    GSS_REQUIRE(ctx, Y && X && F >= 1 && T >= 1, GSS_ERR_INVALID, "gss_wpe: bad arguments");
    GSS_REQUIRE(ctx, D >= 1 && D <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED,
                "gss_wpe: D=%d outside [1, %d]", D, GSS_MAX_CHANNELS);
    GSS_TRY(check_wpe_args(ctx, "gss_wpe", taps, delay, iterations, psd_context));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    GSS_TRY(arena_reserve(ctx, wpe_workspace_bytes(F, T, D, taps, delay)));
    return wpe_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, taps, delay, iterations,
                   psd_context, reinterpret_cast<cplx *>(X));
}

// gss_wpe_arrays with more than one array: input and output regrouped by array, (F A, T, C)
struct WpeArraysWork {
    cplx *Yg, *Xg;
};
static WpeArraysWork wpe_arrays_blocks(Workspace &ws, int F, int64_t T, int D) {
    WpeArraysWork k;
    k.Yg = ws.take<cplx>((size_t)F * T * D, "wpe arrays Y by array");
    k.Xg = ws.take<cplx>((size_t)F * T * D, "wpe arrays X by array");
    return k;
}

extern "C" int gss_wpe_arrays(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int A, int C,
                              int taps, int delay, int iterations, int psd_context, gss_cplx *X) {
    GSS_ENTER_VARIANTS(ctx);
    GSS_REQUIRE(ctx, Y && X && F >= 1 && T >= 1 && A >= 1 && C >= 1, GSS_ERR_INVALID,
                "gss_wpe_arrays: bad arguments");
    const int D = A * C;
    GSS_REQUIRE(ctx, D <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED,
                "gss_wpe_arrays: A * C = %d outside [1, %d]", D, GSS_MAX_CHANNELS);
    GSS_TRY(check_wpe_args(ctx, "gss_wpe_arrays", taps, delay, iterations, psd_context));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    if (A == 1) {       // one array: gss_wpe itself
        GSS_REQUIRE(ctx, X != Y || iterations == 0, GSS_ERR_INVALID,
                    "gss_wpe_arrays: X must not alias Y");
        GSS_TRY(arena_reserve(ctx, wpe_workspace_bytes(F, T, D, taps, delay)));
        return wpe_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, taps, delay, iterations,
                       psd_context, reinterpret_cast<cplx *>(X));
    }
    Workspace sizing;
    wpe_arrays_blocks(sizing, F, T, D);
    GSS_TRY(arena_reserve(ctx, sizing.bytes + wpe_workspace_bytes(F * A, T, C, taps, delay) +
                                   (1 << 16)));
    Workspace ws(ctx);
    const WpeArraysWork k = wpe_arrays_blocks(ws, F, T, D);
    GSS_TRY(ws.status("gss_wpe_arrays"));
    GSS_TRY(wpe_arrays_regroup_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, A, C, true, k.Yg));
    GSS_TRY(wpe_run(ctx, k.Yg, F * A, T, C, taps, delay, iterations, psd_context, k.Xg, -1, F * A));
    return wpe_arrays_regroup_run(ctx, k.Xg, F, T, A, C, false, reinterpret_cast<cplx *>(X));
}

// The online WPE argument rule, before any launch; fills n = taps * C.
static int check_wpe_online(gss_ctx *ctx, const char *what, int F, int A, int C, int taps, int delay,
                            double alpha) {
    GSS_REQUIRE(ctx, F >= 1, GSS_ERR_INVALID, "%s: F = %d is smaller than 1", what, F);
    GSS_REQUIRE(ctx, A >= 1, GSS_ERR_INVALID, "%s: A = %d is smaller than 1", what, A);
    GSS_REQUIRE(ctx, C >= 1, GSS_ERR_INVALID, "%s: C = %d is smaller than 1", what, C);
    GSS_REQUIRE(ctx, taps >= 1, GSS_ERR_INVALID, "%s: taps = %d is smaller than 1", what, taps);
    GSS_REQUIRE(ctx, delay >= 0, GSS_ERR_INVALID, "%s: delay = %d is negative", what, delay);
    GSS_REQUIRE(ctx, delay < (1 << 20), GSS_ERR_INVALID, "%s: delay = %d is not below 2^20", what,
                delay);
    GSS_REQUIRE(ctx, std::isfinite(alpha) && alpha > 0.0 && alpha <= 1.0, GSS_ERR_INVALID,
                "%s: alpha = %g outside (0, 1]", what, alpha);
    GSS_REQUIRE(ctx, (int64_t)A * C <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED,
                "%s: A * C = %lld outside [1, %d]", what, (long long)A * C, GSS_MAX_CHANNELS);
    GSS_REQUIRE(ctx, (int64_t)taps * C <= 512, GSS_ERR_UNSUPPORTED,
                "%s: n = taps * C = %lld is larger than 512", what, (long long)taps * C);
    return GSS_OK;
}

static int check_wpe_online_state(gss_ctx *ctx, const char *what, const gss_wpe_online_state *s) {
    GSS_REQUIRE(ctx, s->inv_cov_dev, GSS_ERR_INVALID, "%s: state->inv_cov_dev is NULL", what);
    GSS_REQUIRE(ctx, s->filter_dev, GSS_ERR_INVALID, "%s: state->filter_dev is NULL", what);
    GSS_REQUIRE(ctx, s->history_dev, GSS_ERR_INVALID, "%s: state->history_dev is NULL", what);
    return GSS_OK;
}

extern "C" int gss_wpe_online_init(gss_ctx *ctx, int F, int A, int C, int taps, int delay,
                                   const gss_wpe_online_state *state) {
    GSS_ENTER(ctx);
    GSS_REQUIRE(ctx, state, GSS_ERR_INVALID, "gss_wpe_online_init: state is NULL");
    GSS_TRY(check_wpe_online_state(ctx, "gss_wpe_online_init", state));
    GSS_TRY(check_wpe_online(ctx, "gss_wpe_online_init", F, A, C, taps, delay, 1.0));
    return wpe_online_init_run(ctx, F, A, C, taps, delay, reinterpret_cast<cplx *>(state->inv_cov_dev),
                               reinterpret_cast<cplx *>(state->filter_dev),
                               reinterpret_cast<cplx *>(state->history_dev));
}

extern "C" int gss_wpe_online(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int A, int C,
                              int taps, int delay, double alpha, const gss_wpe_online_state *state,
                              gss_cplx *X) {
    GSS_ENTER_VARIANTS(ctx);
    GSS_REQUIRE(ctx, Y, GSS_ERR_INVALID, "gss_wpe_online: Y_dev is NULL");
    GSS_REQUIRE(ctx, X, GSS_ERR_INVALID, "gss_wpe_online: X_dev is NULL");
    GSS_REQUIRE(ctx, X != Y, GSS_ERR_INVALID, "gss_wpe_online: X_dev must not alias Y_dev");
    GSS_REQUIRE(ctx, T >= 0, GSS_ERR_INVALID, "gss_wpe_online: T = %lld is negative", (long long)T);
    if (state) GSS_TRY(check_wpe_online_state(ctx, "gss_wpe_online", state));
    GSS_TRY(check_wpe_online(ctx, "gss_wpe_online", F, A, C, taps, delay, alpha));
    GSS_TRY(check_stft_bins(ctx, F, T, A * C));
    const bool force_mem = gss_variant_set("wpe_online_mem");
    if (T == 0) return GSS_OK;
    GSS_TRY(arena_reserve(ctx, wpe_online_workspace_bytes(F, T, A, C, taps, delay, state == nullptr)));
    return wpe_online_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, A, C, taps, delay, alpha,
                          state ? reinterpret_cast<cplx *>(state->inv_cov_dev) : nullptr,
                          state ? reinterpret_cast<cplx *>(state->filter_dev) : nullptr,
                          state ? reinterpret_cast<cplx *>(state->history_dev) : nullptr,
                          reinterpret_cast<cplx *>(X), force_mem);
}

extern "C" int gss_wpe_inverse_power(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                                     int psd_context, double *inverse_power) {
    GSS_ENTER_VARIANTS(ctx);
    GSS_REQUIRE(ctx, Y && inverse_power && F >= 1 && T >= 1 && psd_context >= 0, GSS_ERR_INVALID,
                "gss_wpe_inverse_power: bad arguments");
    GSS_REQUIRE(ctx, D >= 1 && D <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED,
                "gss_wpe_inverse_power: D=%d outside [1, %d]", D, GSS_MAX_CHANNELS);
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    GSS_TRY(arena_reserve(ctx, wpe_inverse_power_workspace_bytes(F, T)));
    return wpe_inverse_power_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, psd_context,
                                 inverse_power);
}

static int check_cacgmm_args(gss_ctx *ctx, int D, int K, int iterations, int post) {
    GSS_REQUIRE(ctx, D >= 2 && D <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED,
                "cacgmm: D=%d outside [2, %d]", D, GSS_MAX_CHANNELS);
    GSS_TRY(check_class_count(ctx, K));
    GSS_REQUIRE(ctx, iterations >= 1 && post >= 0, GSS_ERR_INVALID,
                "cacgmm: iterations=%d iterations_post=%d", iterations, post);
    return GSS_OK;
}

extern "C" int gss_cacgmm(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                          const uint8_t *act, int K, int iterations, int post,
                          double *gamma) {
    GSS_ENTER_VARIANTS(ctx);
    GSS_REQUIRE(ctx, Y && act && gamma && F >= 1 && T >= 1, GSS_ERR_INVALID,
                "gss_cacgmm: bad arguments");
    GSS_TRY(check_cacgmm_args(ctx, D, K, iterations, post));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    GSS_TRY(arena_reserve(ctx, cacgmm_workspace_bytes(F, T, D, K)));
    return cacgmm_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D,
                      em_guide_from_activity(act, T), K, iterations, post, gamma);
}

static int check_mask_strides(gss_ctx *ctx, const gss_guidance *g, int K, int64_t T) {
    GSS_REQUIRE(ctx, g->mask_k_stride >= T, GSS_ERR_INVALID,
                "guidance: mask_k_stride %lld is smaller than T = %lld",
                (long long)g->mask_k_stride, (long long)T);
    GSS_REQUIRE(ctx, g->mask_f_stride == 0 || g->mask_f_stride >= K * g->mask_k_stride,
                GSS_ERR_INVALID, "guidance: mask_f_stride %lld is smaller than K * "
                "mask_k_stride = %lld", (long long)g->mask_f_stride,
                (long long)(K * g->mask_k_stride));
    return GSS_OK;
}

// The descriptor's rules (include/gss_hip.h) -> the EM's view of it.  The values behind the
// pointers are not looked at.
static int check_guidance(gss_ctx *ctx, const gss_guidance *g, int K, int64_t T, EmGuide *out) {
    GSS_REQUIRE(ctx, g, GSS_ERR_INVALID, "guidance is NULL");
    GSS_REQUIRE(ctx, g->init_dev || g->mask_dev, GSS_ERR_INVALID,
                "guidance: init_dev and mask_dev are both NULL");
    if (g->init_dev) {
        GSS_REQUIRE(ctx, g->init_k_stride >= T, GSS_ERR_INVALID,
                    "guidance: init_k_stride %lld is smaller than T = %lld",
                    (long long)g->init_k_stride, (long long)T);
        GSS_REQUIRE(ctx, g->init_f_stride == 0 || g->init_f_stride >= K * g->init_k_stride,
                    GSS_ERR_INVALID, "guidance: init_f_stride %lld is smaller than K * "
                    "init_k_stride = %lld", (long long)g->init_f_stride,
                    (long long)(K * g->init_k_stride));
    }
    if (g->mask_dev) GSS_TRY(check_mask_strides(ctx, g, K, T));
    *out = EmGuide{g->init_dev, g->mask_dev, g->init_dev ? g->init_f_stride : 0,
                   g->init_dev ? g->init_k_stride : 0, g->mask_dev ? g->mask_f_stride : 0,
                   g->mask_dev ? g->mask_k_stride : 0};
    return GSS_OK;
}

extern "C" int gss_cacgmm_guided(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                                 const gss_guidance *g, int K, int iterations, int post,
                                 double *gamma) {
    GSS_ENTER_VARIANTS(ctx);
    GSS_REQUIRE(ctx, Y && gamma && F >= 1 && T >= 1, GSS_ERR_INVALID,
                "gss_cacgmm_guided: bad arguments");
    GSS_TRY(check_cacgmm_args(ctx, D, K, iterations, post));
    EmGuide guide;
    GSS_TRY(check_guidance(ctx, g, K, T, &guide));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    GSS_TRY(arena_reserve(ctx, cacgmm_workspace_bytes(F, T, D, K)));
    return cacgmm_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, guide, K, iterations, post,
                      gamma);
}

// pb_bss weight_constant_axis=-3: one prior[k, t] for all frequencies in place of pi[f, k]
extern "C" int gss_cacgmm_shared_prior(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                                       const gss_guidance *g, int K, int iterations, int post,
                                       double *gamma, double *prior) {
    GSS_ENTER_VARIANTS(ctx);
    GSS_REQUIRE(ctx, Y && gamma && F >= 1 && T >= 1, GSS_ERR_INVALID,
                "gss_cacgmm_shared_prior: bad arguments");
    GSS_TRY(check_cacgmm_args(ctx, D, K, iterations, post));
    EmGuide guide;
    GSS_TRY(check_guidance(ctx, g, K, T, &guide));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    GSS_TRY(arena_reserve(ctx, cacgmm_workspace_bytes(F, T, D, K, /*one_block=*/true) +
                                   cacgmm_prior_workspace_bytes(F, T, K)));
    // the schedule of cacgmm_run: fit, post - 1 unmasked iterations, predict (masked for post 0)
    EmSchedule s;
    s.iterations = iterations;
    s.model_iterations = std::max(post - 1, 0);
    s.predict_masked = post == 0;
    s.gamma = gamma;
    s.shared_prior = true;
    s.prior = prior;
    return cacgmm_schedule_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, guide, K, s);
}

// ------------------------------------------------------------------ the model as an object
// The mask of a guidance that may be absent (fit(initialization=model), predict): NULL or no
// mask = unmasked; the initialisation's fields are not read.
static int check_mask_guidance(gss_ctx *ctx, const gss_guidance *g, int K, int64_t T, EmGuide *out) {
    *out = EmGuide{};
    if (!g || !g->mask_dev) return GSS_OK;
    GSS_TRY(check_mask_strides(ctx, g, K, T));
    out->mask = g->mask_dev;
    out->mask_f_stride = g->mask_f_stride;
    out->mask_k_stride = g->mask_k_stride;
    return GSS_OK;
}

static int check_model(gss_ctx *ctx, const gss_cacgmm_model *m, const char *name) {
    GSS_REQUIRE(ctx, m, GSS_ERR_INVALID, "%s is NULL", name);
    GSS_REQUIRE(ctx, m->precision_dev, GSS_ERR_INVALID, "%s: precision_dev is NULL", name);
    GSS_REQUIRE(ctx, m->log_det_dev, GSS_ERR_INVALID, "%s: log_det_dev is NULL", name);
    GSS_REQUIRE(ctx, m->weight_dev, GSS_ERR_INVALID, "%s: weight_dev is NULL", name);
    return GSS_OK;
}

static EmModel em_model(const gss_cacgmm_model *m) {
    return EmModel{reinterpret_cast<cplx *>(m->precision_dev), m->log_det_dev, m->weight_dev};
}

extern "C" int gss_cacgmm_fit(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                              const gss_guidance *g, int K, int iterations,
                              const gss_cacgmm_model *init_model,
                              const gss_cacgmm_model *model_out) {
    GSS_ENTER_VARIANTS(ctx);
    GSS_REQUIRE(ctx, Y && F >= 1 && T >= 1, GSS_ERR_INVALID, "gss_cacgmm_fit: bad arguments");
    GSS_TRY(check_cacgmm_args(ctx, D, K, 1, 0));
    GSS_REQUIRE(ctx, iterations >= 0 && (iterations >= 1 || init_model), GSS_ERR_INVALID,
                "gss_cacgmm_fit: iterations=%d%s", iterations,
                iterations == 0 ? " needs an init_model to copy" : "");
    GSS_TRY(check_model(ctx, model_out, "model_out"));
    EmGuide guide;
    if (init_model) {
        GSS_TRY(check_model(ctx, init_model, "init_model"));
        GSS_TRY(check_mask_guidance(ctx, g, K, T, &guide));
    } else {
        GSS_TRY(check_guidance(ctx, g, K, T, &guide));
    }
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    if (iterations == 0) {
        // fit(initialization=model, iterations=0) is the model
        const size_t fk = (size_t)F * K;
        if (model_out->precision_dev != init_model->precision_dev)
            GSS_HIP_CHECK(ctx, hipMemcpyAsync(model_out->precision_dev, init_model->precision_dev,
                                              sizeof(cplx) * fk * D * D, hipMemcpyDeviceToDevice,
                                              ctx->stream));
        if (model_out->log_det_dev != init_model->log_det_dev)
            GSS_HIP_CHECK(ctx, hipMemcpyAsync(model_out->log_det_dev, init_model->log_det_dev,
                                              sizeof(double) * fk, hipMemcpyDeviceToDevice,
                                              ctx->stream));
        if (model_out->weight_dev != init_model->weight_dev)
            GSS_HIP_CHECK(ctx, hipMemcpyAsync(model_out->weight_dev, init_model->weight_dev,
                                              sizeof(double) * fk, hipMemcpyDeviceToDevice,
                                              ctx->stream));
        return GSS_OK;
    }
    GSS_TRY(arena_reserve(ctx, cacgmm_workspace_bytes(F, T, D, K)));
    const EmModel in = init_model ? em_model(init_model) : EmModel{}, out = em_model(model_out);
    EmSchedule s;
    if (init_model) {
        s.import_model = &in;
        s.model_iterations = iterations;
        s.model_masked = true;
    } else {
        s.iterations = iterations;
    }
    s.export_model = &out;
    return cacgmm_schedule_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, guide, K, s);
}

extern "C" int gss_cacgmm_predict(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                                  const gss_cacgmm_model *model, int K, const gss_guidance *g,
                                  double *gamma, double *loglik) {
    GSS_ENTER_VARIANTS(ctx);
    GSS_REQUIRE(ctx, Y && F >= 1 && T >= 1, GSS_ERR_INVALID, "gss_cacgmm_predict: bad arguments");
    GSS_TRY(check_cacgmm_args(ctx, D, K, 1, 0));
    GSS_TRY(check_model(ctx, model, "model"));
    GSS_REQUIRE(ctx, gamma || loglik, GSS_ERR_INVALID,
                "gss_cacgmm_predict: gamma_dev and loglik_dev are both NULL");
    EmGuide guide;
    GSS_TRY(check_mask_guidance(ctx, g, K, T, &guide));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    // the workspace of THIS call's (F, T, D, K): a predict may see more frames than any fit did
    GSS_TRY(arena_reserve(ctx, cacgmm_workspace_bytes(F, T, D, K)));
    const EmModel in = em_model(model);
    EmSchedule s;
    s.import_model = &in;
    s.predict_masked = true;
    s.gamma = gamma;
    s.loglik = loglik;
    return cacgmm_schedule_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, guide, K, s);
}

// ------------------------------------------------------------------ permutation alignment
extern "C" int gss_cacgmm_align(gss_ctx *ctx, const double *gamma, int F, int K, int64_t T,
                                const gss_align_plan *plan, int32_t *mapping, double *aligned,
                                double *activity) {
    GSS_ENTER(ctx);
    const char *what = "gss_cacgmm_align";
    GSS_REQUIRE(ctx, gamma, GSS_ERR_INVALID, "%s: gamma_dev is NULL", what);
    GSS_REQUIRE(ctx, mapping, GSS_ERR_INVALID, "%s: mapping_dev is NULL", what);
    GSS_REQUIRE(ctx, plan, GSS_ERR_INVALID, "%s: plan is NULL", what);
    GSS_REQUIRE(ctx, plan->iterations && plan->start && plan->end, GSS_ERR_INVALID,
                "%s: plan: an array (iterations, start or end) is NULL", what);
    GSS_REQUIRE(ctx, F >= 1, GSS_ERR_INVALID, "%s: F=%d is smaller than 1", what, F);
    GSS_REQUIRE(ctx, T >= 1, GSS_ERR_INVALID, "%s: T=%lld is smaller than 1", what, (long long)T);
    GSS_REQUIRE(ctx, K >= 1, GSS_ERR_INVALID, "%s: K=%d is smaller than 1", what, K);
    GSS_REQUIRE(ctx, K <= GSS_ALIGN_MAX_CLASSES, GSS_ERR_UNSUPPORTED,
                "%s: K=%d is larger than %d (the search is exhaustive)", what, K,
                GSS_ALIGN_MAX_CLASSES);
    GSS_REQUIRE(ctx, plan->entries >= 1, GSS_ERR_INVALID, "%s: plan: entries=%d is smaller than 1",
                what, (int)plan->entries);
    for (int e = 0; e < plan->entries; ++e) {
        GSS_REQUIRE(ctx, plan->iterations[e] >= 1, GSS_ERR_INVALID,
                    "%s: plan entry %d: iterations=%d is smaller than 1", what, e,
                    (int)plan->iterations[e]);
        GSS_REQUIRE(ctx, 0 <= plan->start[e] && plan->start[e] < plan->end[e] && plan->end[e] <= F,
                    GSS_ERR_INVALID, "%s: plan entry %d: not 0 <= start=%d < end=%d <= F=%d", what,
                    e, (int)plan->start[e], (int)plan->end[e], F);
    }
    GSS_REQUIRE(ctx, aligned != gamma, GSS_ERR_INVALID, "%s: aligned_dev is gamma_dev", what);
    GSS_TRY(arena_reserve(ctx, cacgmm_align_workspace_bytes(F, K, T, plan, activity && !aligned)));
    return cacgmm_align_run(ctx, gamma, F, K, T, plan, mapping, aligned, activity);
}

extern "C" int gss_cacgmm_model_permute(gss_ctx *ctx, const gss_cacgmm_model *model, int F, int K,
                                        int D, const int32_t *mapping,
                                        const gss_cacgmm_model *model_out) {
    GSS_ENTER(ctx);
    const char *what = "gss_cacgmm_model_permute";
    GSS_TRY(check_model(ctx, model, "model"));
    GSS_TRY(check_model(ctx, model_out, "model_out"));
    GSS_REQUIRE(ctx, mapping, GSS_ERR_INVALID, "%s: mapping_dev is NULL", what);
    GSS_REQUIRE(ctx, F >= 1, GSS_ERR_INVALID, "%s: F=%d is smaller than 1", what, F);
    GSS_REQUIRE(ctx, K >= 1, GSS_ERR_INVALID, "%s: K=%d is smaller than 1", what, K);
    GSS_REQUIRE(ctx, D >= 1, GSS_ERR_INVALID, "%s: D=%d is smaller than 1", what, D);
    GSS_REQUIRE(ctx, K <= GSS_MAX_CLASSES, GSS_ERR_UNSUPPORTED, "%s: K=%d is larger than %d", what,
                K, GSS_MAX_CLASSES);
    GSS_REQUIRE(ctx, D <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED, "%s: D=%d is larger than %d", what,
                D, GSS_MAX_CHANNELS);
    const void *in[3] = {model->precision_dev, model->log_det_dev, model->weight_dev};
    const void *out[3] = {model_out->precision_dev, model_out->log_det_dev, model_out->weight_dev};
    for (const void *o : out)
        for (const void *i : in)
            GSS_REQUIRE(ctx, o != i, GSS_ERR_INVALID,
                        "%s: model_out shares a buffer with model (the gather is not in place)", what);
    return cacgmm_model_permute_run(ctx, em_model(model), F, K, D, mapping, em_model(model_out));
}

// ------------------------------------------------------------------ cross-window linking
extern "C" int gss_cacgmm_link(gss_ctx *ctx, const double *prev, int64_t T_prev,
                               int64_t prev_begin, const double *cur, int64_t T_cur,
                               int64_t cur_begin, int64_t L, int F, int K, int32_t *mapping,
                               double *scores) {
    GSS_ENTER(ctx);
    const char *what = "gss_cacgmm_link";
    GSS_REQUIRE(ctx, prev, GSS_ERR_INVALID, "%s: prev_dev is NULL", what);
    GSS_REQUIRE(ctx, cur, GSS_ERR_INVALID, "%s: cur_dev is NULL", what);
    GSS_REQUIRE(ctx, mapping, GSS_ERR_INVALID, "%s: mapping_dev is NULL", what);
    GSS_REQUIRE(ctx, scores, GSS_ERR_INVALID, "%s: scores_dev is NULL", what);
    GSS_REQUIRE(ctx, F >= 1, GSS_ERR_INVALID, "%s: F=%d is smaller than 1", what, F);
    GSS_REQUIRE(ctx, K >= 1, GSS_ERR_INVALID, "%s: K=%d is smaller than 1", what, K);
    GSS_REQUIRE(ctx, L >= 1, GSS_ERR_INVALID, "%s: L=%lld is smaller than 1", what, (long long)L);
    GSS_REQUIRE(ctx, K <= GSS_ALIGN_MAX_CLASSES, GSS_ERR_UNSUPPORTED,
                "%s: K=%d is larger than %d (the search is exhaustive)", what, K,
                GSS_ALIGN_MAX_CLASSES);
    // (begin <= T - L, not begin + L <= T: no overflow for any int64 argument)
    GSS_REQUIRE(ctx, prev_begin >= 0 && L <= T_prev && prev_begin <= T_prev - L, GSS_ERR_INVALID,
                "%s: prev frames [%lld, %lld + %lld) outside [0, T_prev=%lld)", what,
                (long long)prev_begin, (long long)prev_begin, (long long)L, (long long)T_prev);
    GSS_REQUIRE(ctx, cur_begin >= 0 && L <= T_cur && cur_begin <= T_cur - L, GSS_ERR_INVALID,
                "%s: cur frames [%lld, %lld + %lld) outside [0, T_cur=%lld)", what,
                (long long)cur_begin, (long long)cur_begin, (long long)L, (long long)T_cur);
    GSS_TRY(arena_reserve(ctx, cacgmm_link_workspace_bytes(F, K)));
    return cacgmm_link_run(ctx, prev, T_prev, prev_begin, cur, T_cur, cur_begin, L, F, K, mapping,
                           scores);
}

extern "C" int gss_cacgmm_link_gather(gss_ctx *ctx, const double *gamma, int F, int K, int64_t T,
                                      const int32_t *mapping, double *out) {
    GSS_ENTER(ctx);
    const char *what = "gss_cacgmm_link_gather";
    GSS_REQUIRE(ctx, gamma, GSS_ERR_INVALID, "%s: gamma_dev is NULL", what);
    GSS_REQUIRE(ctx, mapping, GSS_ERR_INVALID, "%s: mapping_dev is NULL", what);
    GSS_REQUIRE(ctx, out, GSS_ERR_INVALID, "%s: out_dev is NULL", what);
    GSS_REQUIRE(ctx, F >= 1, GSS_ERR_INVALID, "%s: F=%d is smaller than 1", what, F);
    GSS_REQUIRE(ctx, K >= 1, GSS_ERR_INVALID, "%s: K=%d is smaller than 1", what, K);
    GSS_REQUIRE(ctx, T >= 1, GSS_ERR_INVALID, "%s: T=%lld is smaller than 1", what, (long long)T);
    GSS_REQUIRE(ctx, out != gamma, GSS_ERR_INVALID, "%s: out_dev is gamma_dev", what);
    GSS_REQUIRE(ctx, K <= GSS_MAX_CLASSES, GSS_ERR_UNSUPPORTED, "%s: K=%d is larger than %d", what,
                K, GSS_MAX_CLASSES);
    return cacgmm_link_gather_run(ctx, gamma, F, K, T, mapping, out);
}

extern "C" int gss_masks_from_posteriors(gss_ctx *ctx, const double *gamma, int F, int K,
                                         int64_t T, int target, int drop, int64_t sf,
                                         int64_t ef, double *mx, double *mn) {
    GSS_ENTER(ctx);
    GSS_REQUIRE(ctx, gamma && mx && mn && F >= 1 && T >= 1 && K >= 1, GSS_ERR_INVALID,
                "gss_masks_from_posteriors: bad arguments");
    GSS_TRY(check_target_index(ctx, target, K));
    return masks_from_posteriors_run(ctx, gamma, F, K, T, target, drop, sf, ef, mx, mn);
}

extern "C" int gss_mvdr_souden(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                               const double *mx, const double *mn, int ban, gss_cplx *Xhat,
                               int32_t *ref) {
    GSS_ENTER(ctx);
    GSS_REQUIRE(ctx, Y && mx && mn && Xhat && F >= 1 && T >= 1, GSS_ERR_INVALID,
                "gss_mvdr_souden: bad arguments");
    GSS_TRY(check_bf_channels(ctx, D));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    GSS_TRY(arena_reserve(ctx, mvdr_workspace_bytes(F, T, D)));
    return mvdr_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, mx, mn, ban,
                    reinterpret_cast<cplx *>(Xhat), ref);
}

extern "C" int gss_mvdr_souden_ref(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                                   const double *mx, const double *mn, int ban, int ref_channel,
                                   gss_cplx *Xhat) {
    GSS_ENTER(ctx);
    GSS_REQUIRE(ctx, Y && mx && mn && Xhat && F >= 1 && T >= 1, GSS_ERR_INVALID,
                "gss_mvdr_souden_ref: bad arguments");
    GSS_TRY(check_bf_channels(ctx, D));
    GSS_REQUIRE(ctx, ref_channel >= 0 && ref_channel < D, GSS_ERR_INVALID,
                "ref_channel %d outside [0, %d)", ref_channel, D);
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    GSS_TRY(arena_reserve(ctx, mvdr_workspace_bytes(F, T, D)));
    return mvdr_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, mx, mn, ban,
                    reinterpret_cast<cplx *>(Xhat), nullptr, /*gev=*/0, ref_channel);
}

// One status word of the last call (gss_ctx::status_host), after the context's stream has drained.
template <typename Out>
static int read_status_word(gss_ctx *ctx, int word, Out *out, const char *entry) {
    GSS_ENTER(ctx);
    GSS_REQUIRE(ctx, out, GSS_ERR_INVALID, "%s: NULL", entry);
    GSS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *out = __atomic_load_n(ctx->status_host + word, __ATOMIC_ACQUIRE);
    return GSS_OK;
}

extern "C" int gss_last_ref_channel(gss_ctx *ctx, int32_t *ref_channel) {
    return read_status_word(ctx, GSS_STATUS_REF_CHANNEL, ref_channel, "gss_last_ref_channel");
}

extern "C" int gss_last_ref_channels(gss_ctx *ctx, int32_t *ref_channels, int S) {
    GSS_ENTER(ctx);
    GSS_REQUIRE(ctx, ref_channels, GSS_ERR_INVALID, "gss_last_ref_channels: NULL");
    const int have = ctx->last_targets > 0 ? ctx->last_targets : 1;
    GSS_REQUIRE(ctx, S >= 1 && S <= have, GSS_ERR_INVALID,
                "gss_last_ref_channels: S=%d, the last beamformer run had %d target(s)", S, have);
    GSS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const int32_t *words = ctx->last_targets > 0 ? ctx->status_host + GSS_STATUS_TARGETS
                                                 : ctx->status_host;
    for (int s = 0; s < S; ++s) ref_channels[s] = __atomic_load_n(words + s, __ATOMIC_ACQUIRE);
    return GSS_OK;
}

extern "C" int gss_last_wpe_zero_pivots(gss_ctx *ctx, int64_t *count) {
    return read_status_word(ctx, GSS_STATUS_WPE_ZERO_PIVOTS, count, "gss_last_wpe_zero_pivots");
}

extern "C" int gss_last_align_moved(gss_ctx *ctx, int64_t *count) {
    return read_status_word(ctx, GSS_STATUS_ALIGN_MOVED, count, "gss_last_align_moved");
}

static int check_segments(gss_ctx *ctx, const gss_bf_segments *seg, const char *what) {
    GSS_REQUIRE(ctx, seg, GSS_ERR_INVALID, "%s: seg is NULL", what);
    GSS_REQUIRE(ctx, seg->segment_frames >= 64 && seg->segment_frames % 64 == 0, GSS_ERR_INVALID,
                "%s: segment_frames = %lld is not a positive multiple of 64", what,
                (long long)seg->segment_frames);
    GSS_REQUIRE(ctx, seg->context_segments >= 0, GSS_ERR_INVALID,
                "%s: context_segments = %d is negative", what, (int)seg->context_segments);
    GSS_REQUIRE(ctx, std::isfinite(seg->min_mass) && seg->min_mass >= 0.0, GSS_ERR_INVALID,
                "%s: min_mass = %g is negative or not finite", what, seg->min_mass);
    return GSS_OK;
}

extern "C" int gss_mvdr_souden_segments(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                                        const double *mx, const double *mn, int ban,
                                        int ref_channel, const gss_bf_segments *seg,
                                        gss_cplx *Xhat, int32_t *ref) {
    GSS_ENTER(ctx);
    GSS_REQUIRE(ctx, Y && mx && mn && Xhat && F >= 1 && T >= 1, GSS_ERR_INVALID,
                "gss_mvdr_souden_segments: bad arguments");
    GSS_TRY(check_bf_channels(ctx, D));
    GSS_REQUIRE(ctx, ref_channel >= -1 && ref_channel < D, GSS_ERR_INVALID,
                "ref_channel %d outside [-1, %d)", ref_channel, D);
    GSS_TRY(check_segments(ctx, seg, "gss_mvdr_souden_segments"));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    GSS_TRY(arena_reserve(ctx, mvdr_segments_workspace_bytes(F, T, D, seg->segment_frames)));
    return mvdr_segments_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, mx, mn, ban, *seg,
                             reinterpret_cast<cplx *>(Xhat), ref, ref_channel);
}

extern "C" int gss_last_segment_fallbacks(gss_ctx *ctx, int64_t *count) {
    return read_status_word(ctx, GSS_STATUS_SEGMENT_FALLBACKS, count, "gss_last_segment_fallbacks");
}

// The online MVDR argument rule, before any launch.
static int check_bf_online(gss_ctx *ctx, const char *what, const gss_bf_online *cfg, int D) {
    GSS_REQUIRE(ctx, cfg, GSS_ERR_INVALID, "%s: cfg is NULL", what);
    GSS_REQUIRE(ctx, D >= 1 && D <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED, "%s: D = %d outside [1, %d]",
                what, D, GSS_MAX_CHANNELS);
    GSS_REQUIRE(ctx, std::isfinite(cfg->forget) && cfg->forget > 0.0 && cfg->forget <= 1.0,
                GSS_ERR_INVALID, "%s: forget = %g outside (0, 1]", what, cfg->forget);
    GSS_REQUIRE(ctx, std::isfinite(cfg->loading) && cfg->loading > 0.0, GSS_ERR_INVALID,
                "%s: loading = %g is not finite and > 0", what, cfg->loading);
    GSS_REQUIRE(ctx, cfg->ref_channel >= -1 && cfg->ref_channel < D, GSS_ERR_INVALID,
                "%s: ref_channel = %d outside [-1, %d)", what, (int)cfg->ref_channel, D);
    // (the whole-window pass that picks the channel is the reference's beamformer)
    if (cfg->ref_channel < 0) GSS_TRY(check_bf_channels(ctx, D));
    return GSS_OK;
}

static int check_mvdr_online_state(gss_ctx *ctx, const char *what, const gss_mvdr_online_state *s,
                                   int F, int D) {
    GSS_REQUIRE(ctx, s->phi_x, GSS_ERR_INVALID, "%s: state->phi_x is NULL", what);
    GSS_REQUIRE(ctx, s->phi_n, GSS_ERR_INVALID, "%s: state->phi_n is NULL", what);
    GSS_REQUIRE(ctx, s->phi_x != s->phi_n, GSS_ERR_INVALID, "%s: state->phi_x and state->phi_n alias",
                what);
    GSS_REQUIRE(ctx, s->F == F && s->D == D, GSS_ERR_INVALID,
                "%s: state of F = %d, D = %d in a call of F = %d, D = %d", what, (int)s->F, (int)s->D,
                F, D);
    return GSS_OK;
}

extern "C" int gss_mvdr_online_init(gss_ctx *ctx, int F, int D, const gss_cplx *Y, int64_t T,
                                    double loading, gss_mvdr_online_state *state) {
    GSS_ENTER(ctx);
    const char *const what = "gss_mvdr_online_init";
    GSS_REQUIRE(ctx, state, GSS_ERR_INVALID, "%s: state is NULL", what);
    GSS_REQUIRE(ctx, F >= 1, GSS_ERR_INVALID, "%s: F = %d is smaller than 1", what, F);
    GSS_REQUIRE(ctx, D >= 1 && D <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED, "%s: D = %d outside [1, %d]",
                what, D, GSS_MAX_CHANNELS);
    GSS_REQUIRE(ctx, T >= 0, GSS_ERR_INVALID, "%s: T = %lld is negative", what, (long long)T);
    GSS_REQUIRE(ctx, std::isfinite(loading) && loading > 0.0, GSS_ERR_INVALID,
                "%s: loading = %g is not finite and > 0", what, loading);
    GSS_TRY(check_mvdr_online_state(ctx, what, state, F, D));
    if (Y && T > 0) GSS_TRY(check_stft_bins(ctx, F, T, D));
    return mvdr_online_init_run(ctx, F, D, reinterpret_cast<const cplx *>(Y), Y ? T : 0, loading,
                                reinterpret_cast<cplx *>(state->phi_x),
                                reinterpret_cast<cplx *>(state->phi_n));
}

extern "C" int gss_mvdr_online(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                               const double *mx, const double *mn, int ban, const gss_bf_online *cfg,
                               gss_mvdr_online_state *state, gss_cplx *Xhat, gss_cplx *W) {
    GSS_ENTER(ctx);
    const char *const what = "gss_mvdr_online";
    GSS_REQUIRE(ctx, Y, GSS_ERR_INVALID, "%s: Y_dev is NULL", what);
    GSS_REQUIRE(ctx, mx, GSS_ERR_INVALID, "%s: mask_x_dev is NULL", what);
    GSS_REQUIRE(ctx, mn, GSS_ERR_INVALID, "%s: mask_n_dev is NULL", what);
    GSS_REQUIRE(ctx, Xhat, GSS_ERR_INVALID, "%s: Xhat_dev is NULL", what);
    GSS_REQUIRE(ctx, F >= 1, GSS_ERR_INVALID, "%s: F = %d is smaller than 1", what, F);
    GSS_REQUIRE(ctx, T >= 0, GSS_ERR_INVALID, "%s: T = %lld is negative", what, (long long)T);
    GSS_TRY(check_bf_online(ctx, what, cfg, D));
    if (state) GSS_TRY(check_mvdr_online_state(ctx, what, state, F, D));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    if (T == 0) return GSS_OK;
    GSS_TRY(arena_reserve(ctx, mvdr_online_workspace_bytes(F, T, D, state == nullptr,
                                                           cfg->ref_channel < 0)));
    return mvdr_online_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, mx, mn, ban != 0,
                           cfg->forget, cfg->loading, cfg->ref_channel,
                           state ? reinterpret_cast<cplx *>(state->phi_x) : nullptr,
                           state ? reinterpret_cast<cplx *>(state->phi_n) : nullptr,
                           reinterpret_cast<cplx *>(Xhat), T, 1, reinterpret_cast<cplx *>(W));
}

extern "C" int gss_last_mvdr_online_fallbacks(gss_ctx *ctx, int64_t *count) {
    return read_status_word(ctx, GSS_STATUS_MVDR_ONLINE_FALLBACKS, count,
                            "gss_last_mvdr_online_fallbacks");
}

// The online CACGMM argument rules, before any launch.
static int check_em_online_shape(gss_ctx *ctx, const char *what, int F, int K, int D) {
    GSS_REQUIRE(ctx, F >= 1, GSS_ERR_INVALID, "%s: F = %d is smaller than 1", what, F);
    GSS_REQUIRE(ctx, D >= 1 && D <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED, "%s: D = %d outside [1, %d]",
                what, D, GSS_MAX_CHANNELS);
    GSS_REQUIRE(ctx, K >= 1 && K <= GSS_CACGMM_ONLINE_MAX_CLASSES, GSS_ERR_UNSUPPORTED,
                "%s: K = %d outside [1, %d]", what, K, GSS_CACGMM_ONLINE_MAX_CLASSES);
    return GSS_OK;
}

static int check_em_online(gss_ctx *ctx, const char *what, const gss_em_online *cfg) {
    GSS_REQUIRE(ctx, cfg, GSS_ERR_INVALID, "%s: cfg is NULL", what);
    GSS_REQUIRE(ctx, std::isfinite(cfg->forget) && cfg->forget > 0.0 && cfg->forget <= 1.0,
                GSS_ERR_INVALID, "%s: forget = %g outside (0, 1]", what, cfg->forget);
    GSS_REQUIRE(ctx, std::isfinite(cfg->prior_mass) && cfg->prior_mass > 0.0, GSS_ERR_INVALID,
                "%s: prior_mass = %g is not finite and > 0", what, cfg->prior_mass);
    return GSS_OK;
}

static int check_cacgmm_online_state(gss_ctx *ctx, const char *what,
                                     const gss_cacgmm_online_state *s, int F, int K, int D) {
    GSS_REQUIRE(ctx, s->s, GSS_ERR_INVALID, "%s: state->s is NULL", what);
    GSS_REQUIRE(ctx, s->n, GSS_ERR_INVALID, "%s: state->n is NULL", what);
    GSS_REQUIRE(ctx, s->F == F && s->K == K && s->D == D, GSS_ERR_INVALID,
                "%s: state of F = %d, K = %d, D = %d in a call of F = %d, K = %d, D = %d", what,
                (int)s->F, (int)s->K, (int)s->D, F, K, D);
    return GSS_OK;
}

extern "C" int gss_cacgmm_online_init(gss_ctx *ctx, int F, int K, int D, double prior_mass,
                                      const gss_cacgmm_model *model, double model_mass,
                                      gss_cacgmm_online_state *state) {
    GSS_ENTER(ctx);
    const char *const what = "gss_cacgmm_online_init";
    GSS_REQUIRE(ctx, state, GSS_ERR_INVALID, "%s: state is NULL", what);
    GSS_TRY(check_em_online_shape(ctx, what, F, K, D));
    GSS_TRY(check_cacgmm_online_state(ctx, what, state, F, K, D));
    cplx *S = reinterpret_cast<cplx *>(state->s);
    if (!model) {
        GSS_REQUIRE(ctx, std::isfinite(prior_mass) && prior_mass > 0.0, GSS_ERR_INVALID,
                    "%s: prior_mass = %g is not finite and > 0", what, prior_mass);
        return cacgmm_online_fresh_run(ctx, F, K, D, prior_mass, S, state->n);
    }
    GSS_TRY(check_model(ctx, model, "model"));
    GSS_REQUIRE(ctx, std::isfinite(model_mass) && model_mass > 0.0, GSS_ERR_INVALID,
                "%s: model_mass = %g is not finite and > 0", what, model_mass);
    GSS_TRY(arena_reserve(ctx, cacgmm_online_workspace_bytes(F, K, D, false)));
    GSS_TRY(cacgmm_online_from_model_run(ctx, em_model(model), F, K, D, model_mass, S, state->n));
    int32_t bad = 0;
    GSS_TRY(read_status_word(ctx, GSS_STATUS_CACGMM_ONLINE_BAD_MODEL, &bad, what));
    GSS_REQUIRE(ctx, bad == 0, GSS_ERR_INVALID,
                "%s: model: the precision of %d (frequency, class) pairs has no Cholesky factor", what,
                (int)bad);
    return GSS_OK;
}

extern "C" int gss_cacgmm_online(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                                 const gss_guidance *g, int K, const gss_em_online *cfg,
                                 gss_cacgmm_online_state *state, double *gamma) {
    GSS_ENTER(ctx);
    const char *const what = "gss_cacgmm_online";
    GSS_REQUIRE(ctx, Y, GSS_ERR_INVALID, "%s: Y_dev is NULL", what);
    GSS_REQUIRE(ctx, gamma, GSS_ERR_INVALID, "%s: gamma_dev is NULL", what);
    GSS_REQUIRE(ctx, T >= 0, GSS_ERR_INVALID, "%s: T = %lld is negative", what, (long long)T);
    GSS_TRY(check_em_online_shape(ctx, what, F, K, D));
    GSS_TRY(check_em_online(ctx, what, cfg));
    if (state) GSS_TRY(check_cacgmm_online_state(ctx, what, state, F, K, D));
    EmGuide guide;
    GSS_TRY(check_mask_guidance(ctx, g, K, T, &guide));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    if (T == 0) return GSS_OK;
    GSS_TRY(arena_reserve(ctx, cacgmm_online_workspace_bytes(F, K, D, state == nullptr)));
    return cacgmm_online_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, guide, K, cfg->forget,
                             cfg->prior_mass, state ? reinterpret_cast<cplx *>(state->s) : nullptr,
                             state ? state->n : nullptr, gamma);
}

extern "C" int gss_cacgmm_online_model(gss_ctx *ctx, const gss_cacgmm_online_state *state,
                                       const gss_cacgmm_model *model_out) {
    GSS_ENTER(ctx);
    const char *const what = "gss_cacgmm_online_model";
    GSS_REQUIRE(ctx, state, GSS_ERR_INVALID, "%s: state is NULL", what);
    GSS_TRY(check_em_online_shape(ctx, what, state->F, state->K, state->D));
    GSS_TRY(check_cacgmm_online_state(ctx, what, state, state->F, state->K, state->D));
    GSS_TRY(check_model(ctx, model_out, "model_out"));
    GSS_REQUIRE(ctx, (void *)model_out->precision_dev != (void *)state->s &&
                         model_out->log_det_dev != state->n && model_out->weight_dev != state->n,
                GSS_ERR_INVALID, "%s: model_out shares a buffer with the state", what);
    GSS_TRY(arena_reserve(ctx, cacgmm_online_workspace_bytes(state->F, state->K, state->D, false)));
    return cacgmm_online_to_model_run(ctx, reinterpret_cast<const cplx *>(state->s), state->n,
                                      state->F, state->K, state->D, em_model(model_out));
}

extern "C" int gss_last_cacgmm_online_fallbacks(gss_ctx *ctx, int64_t *count) {
    return read_status_word(ctx, GSS_STATUS_CACGMM_ONLINE_FALLBACKS, count,
                            "gss_last_cacgmm_online_fallbacks");
}

extern "C" int gss_wpe_weighted(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D, int taps,
                                int delay, const double *weights, gss_cplx *X) {
    GSS_ENTER_VARIANTS(ctx);
    GSS_REQUIRE(ctx, Y && X && weights && F >= 1 && T >= 1, GSS_ERR_INVALID,
                "gss_wpe_weighted: bad arguments");
    GSS_REQUIRE(ctx, D >= 1 && D <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED,
                "gss_wpe_weighted: D=%d outside [1, %d]", D, GSS_MAX_CHANNELS);
    GSS_TRY(check_wpe_args(ctx, "gss_wpe_weighted", taps, delay, 1, 0, /*fixed_schedule=*/true));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    GSS_TRY(arena_reserve(ctx, wpe_workspace_bytes(F, T, D, taps, delay)));
    const WpeCallerWeights cw{weights, 2, false};
    return wpe_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, taps, delay, 1, 0,
                   reinterpret_cast<cplx *>(X), -1, 0, &cw);
}

static int check_power_floor(gss_ctx *ctx, double floor, const char *what) {
    GSS_REQUIRE(ctx, std::isfinite(floor) && floor > 0.0 && floor <= 1.0, GSS_ERR_INVALID,
                "%s: power_floor = %g outside (0, 1] or not finite", what, floor);
    return GSS_OK;
}

// The descriptor's rules (include/gss_hip.h)
static int check_wpd(gss_ctx *ctx, const gss_bf_wpd *wpd, int D, const char *what) {
    GSS_REQUIRE(ctx, wpd, GSS_ERR_INVALID, "%s: wpd is NULL", what);
    GSS_REQUIRE(ctx, wpd->taps >= 1, GSS_ERR_INVALID, "%s: taps = %d is smaller than 1", what,
                wpd->taps);
    GSS_REQUIRE(ctx, wpd->delay >= 0, GSS_ERR_INVALID, "%s: delay = %d is negative", what,
                wpd->delay);
    GSS_REQUIRE(ctx, wpd->iterations >= 1, GSS_ERR_INVALID, "%s: iterations = %d is smaller than 1",
                what, wpd->iterations);
    GSS_TRY(check_power_floor(ctx, wpd->power_floor, what));
    GSS_TRY(check_bf_channels(ctx, D));
    return GSS_OK;
}

extern "C" int gss_wpd_weights(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                               const double *mask, const gss_cplx *Xhat, const uint8_t *gate,
                               double power_floor, double *weights) {
    GSS_ENTER(ctx);
    GSS_REQUIRE(ctx, weights, GSS_ERR_INVALID, "gss_wpd_weights: weights_dev is NULL");
    GSS_REQUIRE(ctx, Xhat || (Y && mask), GSS_ERR_INVALID,
                "gss_wpd_weights: neither Xhat_dev nor Y_dev with mask_dev");
    GSS_REQUIRE(ctx, F >= 1 && T >= 1, GSS_ERR_INVALID, "gss_wpd_weights: F=%d T=%lld", F,
                (long long)T);
    GSS_TRY(check_bf_channels(ctx, D));
    GSS_TRY(check_power_floor(ctx, power_floor, "gss_wpd_weights"));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    return wpd_weights_run(ctx, reinterpret_cast<const cplx *>(Y), mask,
                           reinterpret_cast<const cplx *>(Xhat), gate, F, T, D, power_floor,
                           weights, nullptr);
}

extern "C" int gss_wpd_souden(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                              const double *mask, const uint8_t *gate, const gss_bf_wpd *wpd,
                              int ref_channel, gss_cplx *Xhat, int32_t *ref) {
    GSS_ENTER_VARIANTS(ctx);
    GSS_REQUIRE(ctx, Y, GSS_ERR_INVALID, "gss_wpd_souden: Y_dev is NULL");
    GSS_REQUIRE(ctx, mask, GSS_ERR_INVALID, "gss_wpd_souden: target_mask_dev is NULL");
    GSS_REQUIRE(ctx, Xhat, GSS_ERR_INVALID, "gss_wpd_souden: Xhat_dev is NULL");
    GSS_REQUIRE(ctx, F >= 1 && T >= 1, GSS_ERR_INVALID, "gss_wpd_souden: F=%d T=%lld", F,
                (long long)T);
    GSS_TRY(check_wpd(ctx, wpd, D, "gss_wpd_souden"));
    GSS_REQUIRE(ctx, ref_channel >= -1 && ref_channel < D, GSS_ERR_INVALID,
                "ref_channel %d outside [-1, %d)", ref_channel, D);
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    GSS_TRY(arena_reserve(ctx, wpd_workspace_bytes(F, T, D, wpd->taps, wpd->delay)));
    return wpd_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, mask, gate, *wpd, ref_channel,
                   reinterpret_cast<cplx *>(Xhat), ref);
}

extern "C" int gss_last_wpd_zero_pivots(gss_ctx *ctx, int64_t *count) {
    return read_status_word(ctx, GSS_STATUS_WPD_ZERO_PIVOTS, count, "gss_last_wpd_zero_pivots");
}

// The descriptor's rules (include/gss_hip.h); K bounds the class indices.
static int check_lcmv(gss_ctx *ctx, const gss_bf_lcmv *lcmv, int K, int target, const char *what) {
    GSS_REQUIRE(ctx, lcmv, GSS_ERR_INVALID, "%s: lcmv is NULL", what);
    GSS_REQUIRE(ctx, std::isfinite(lcmv->min_mass) && lcmv->min_mass >= 0.0, GSS_ERR_INVALID,
                "%s: min_mass = %g is negative or not finite", what, lcmv->min_mass);
    GSS_REQUIRE(ctx, lcmv->interferer >= -1 && lcmv->interferer < K, GSS_ERR_INVALID,
                "%s: interferer = %d outside [-1, %d)", what, (int)lcmv->interferer, K);
    GSS_REQUIRE(ctx, lcmv->interferer != target, GSS_ERR_INVALID,
                "%s: interferer = %d is the target", what, (int)lcmv->interferer);
    return GSS_OK;
}

// (D < 2: g = tr A tr B - tr(A B) is identically 0 on one channel)
static int check_lcmv_channels(gss_ctx *ctx, int D, const char *what) {
    GSS_REQUIRE(ctx, D >= 2, GSS_ERR_INVALID, "%s: D = %d, the LCMV needs at least 2 channels",
                what, D);
    return check_bf_channels(ctx, D);
}

extern "C" int gss_lcmv_souden(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                               const double *mx, const double *mi, const double *mn, int ban,
                               int ref_channel, double min_mass, gss_cplx *Xhat, int32_t *ref) {
    GSS_ENTER(ctx);
    GSS_REQUIRE(ctx, Y && mx && mi && mn && Xhat && F >= 1 && T >= 1, GSS_ERR_INVALID,
                "gss_lcmv_souden: bad arguments");
    GSS_TRY(check_lcmv_channels(ctx, D, "gss_lcmv_souden"));
    GSS_REQUIRE(ctx, std::isfinite(min_mass) && min_mass >= 0.0, GSS_ERR_INVALID,
                "gss_lcmv_souden: min_mass = %g is negative or not finite", min_mass);
    GSS_REQUIRE(ctx, ref_channel >= -1 && ref_channel < D, GSS_ERR_INVALID,
                "ref_channel %d outside [-1, %d)", ref_channel, D);
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    GSS_TRY(arena_reserve(ctx, lcmv_workspace_bytes(F, T, D)));
    return lcmv_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, mx, mi, mn, ban, ref_channel,
                    min_mass, reinterpret_cast<cplx *>(Xhat), ref);
}

extern "C" int gss_lcmv_masks_from_posteriors(gss_ctx *ctx, const double *gamma, int F, int K,
                                              int64_t T, int target, const gss_bf_lcmv *lcmv,
                                              int drop, int64_t sf, int64_t ef, double *mx,
                                              double *mi, double *mn, int32_t *interferer) {
    GSS_ENTER(ctx);
    GSS_REQUIRE(ctx, gamma && mx && mi && mn && F >= 1 && T >= 1, GSS_ERR_INVALID,
                "gss_lcmv_masks_from_posteriors: bad arguments");
    GSS_TRY(check_class_count(ctx, K));
    GSS_TRY(check_target_index(ctx, target, K));
    GSS_TRY(check_lcmv(ctx, lcmv, K, target, "gss_lcmv_masks_from_posteriors"));
    GSS_TRY(arena_reserve(ctx, lcmv_masks_workspace_bytes(F, K)));
    return lcmv_masks_run(ctx, gamma, F, K, T, target, *lcmv, drop, sf, ef, mx, mi, mn,
                          interferer);
}

extern "C" int gss_last_lcmv_interferer(gss_ctx *ctx, int32_t *interferer) {
    return read_status_word(ctx, GSS_STATUS_LCMV_INTERFERER, interferer, "gss_last_lcmv_interferer");
}

extern "C" int gss_last_lcmv_fallbacks(gss_ctx *ctx, int64_t *count) {
    return read_status_word(ctx, GSS_STATUS_LCMV_FALLBACKS, count, "gss_last_lcmv_fallbacks");
}

extern "C" int gss_gev(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D, const double *mx,
                       const double *mn, int ban, gss_cplx *Xhat) {
    GSS_ENTER(ctx);
    GSS_REQUIRE(ctx, Y && mx && mn && Xhat && F >= 1 && T >= 1, GSS_ERR_INVALID,
                "gss_gev: bad arguments");
    GSS_TRY(check_bf_channels(ctx, D));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    GSS_TRY(arena_reserve(ctx, mvdr_workspace_bytes(F, T, D)));
    return mvdr_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, mx, mn, ban,
                    reinterpret_cast<cplx *>(Xhat), nullptr, /*gev=*/1);
}

// The descriptor's rules (include/gss_hip.h); `keep` is checked against D where it is read.
static int check_channel_select(gss_ctx *ctx, const gss_channel_select *sel, int D, bool keep,
                                const char *what) {
    GSS_REQUIRE(ctx, sel, GSS_ERR_INVALID, "%s: sel is NULL", what);
    GSS_REQUIRE(ctx, sel->bank_dev, GSS_ERR_INVALID, "%s: bank_dev is NULL", what);
    GSS_REQUIRE(ctx, sel->bands >= 1 && sel->bands <= 64, GSS_ERR_INVALID,
                "%s: bands = %d outside [1, 64]", what, (int)sel->bands);
    GSS_REQUIRE(ctx, std::isfinite(sel->floor) && sel->floor >= 0.0 && sel->floor < 1.0,
                GSS_ERR_INVALID, "%s: floor = %g is negative, >= 1 or not finite", what,
                sel->floor);
    if (keep)
        GSS_REQUIRE(ctx, sel->keep >= 1 && sel->keep <= D, GSS_ERR_INVALID,
                    "%s: keep = %d outside [1, %d]", what, (int)sel->keep, D);
    return GSS_OK;
}

extern "C" int gss_channel_scores(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                                  const gss_channel_select *sel, double *scores,
                                  double *band_var) {
    GSS_ENTER(ctx);
    GSS_REQUIRE(ctx, Y && scores && F >= 1 && T >= 1, GSS_ERR_INVALID,
                "gss_channel_scores: bad arguments");
    GSS_REQUIRE(ctx, D >= 1 && D <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED,
                "gss_channel_scores: D=%d outside [1, %d]", D, GSS_MAX_CHANNELS);
    GSS_TRY(check_channel_select(ctx, sel, D, false, "gss_channel_scores"));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    GSS_TRY(arena_reserve(ctx, chsel_workspace_bytes(F, T, D, sel->bands)));
    return chsel_scores_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, *sel, scores,
                            band_var);
}

extern "C" int gss_select_channels(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                                   const gss_channel_select *sel, gss_cplx *Ysel,
                                   int32_t *channels) {
    GSS_ENTER(ctx);
    GSS_REQUIRE(ctx, Y && Ysel && F >= 1 && T >= 1, GSS_ERR_INVALID,
                "gss_select_channels: bad arguments");
    GSS_REQUIRE(ctx, D >= 1 && D <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED,
                "gss_select_channels: D=%d outside [1, %d]", D, GSS_MAX_CHANNELS);
    GSS_TRY(check_channel_select(ctx, sel, D, true, "gss_select_channels"));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    GSS_TRY(arena_reserve(ctx, chsel_workspace_bytes(F, T, D, sel->bands)));
    return chsel_select_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, *sel,
                            reinterpret_cast<cplx *>(Ysel), channels);
}

extern "C" int gss_last_selected_channels(gss_ctx *ctx, int32_t *channels, int n) {
    GSS_ENTER(ctx);
    GSS_REQUIRE(ctx, channels, GSS_ERR_INVALID, "gss_last_selected_channels: NULL");
    GSS_REQUIRE(ctx, n >= 1 && n <= ctx->last_selected, GSS_ERR_INVALID,
                "gss_last_selected_channels: n=%d, the last selection kept %d channel(s)", n,
                ctx->last_selected);
    GSS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const int32_t *words = ctx->status_host + GSS_STATUS_CHANNELS;
    for (int j = 0; j < n; ++j) channels[j] = __atomic_load_n(words + j, __ATOMIC_ACQUIRE);
    return GSS_OK;
}

// The argument rules of the posterior activity (include/gss_hip.h), shared by both entries.
static int check_activity_sizes(gss_ctx *ctx, int K, int D, const char *what) {
    GSS_REQUIRE(ctx, K >= 1 && K <= GSS_MAX_CLASSES, GSS_ERR_INVALID, "%s: K=%d outside [1, %d]",
                what, K, GSS_MAX_CLASSES);
    GSS_REQUIRE(ctx, D >= 1 && D <= GSS_MAX_CHANNELS, GSS_ERR_INVALID, "%s: D=%d outside [1, %d]",
                what, D, GSS_MAX_CHANNELS);
    return GSS_OK;
}

extern "C" int gss_posterior_activity(gss_ctx *ctx, const gss_cplx *Y, const double *gamma, int F,
                                      int K, int64_t T, int D, const double *freq_weights,
                                      double *scores, double *power) {
    GSS_ENTER(ctx);
    const char *what = "gss_posterior_activity";
    GSS_REQUIRE(ctx, Y, GSS_ERR_INVALID, "%s: Y_dev is NULL", what);
    GSS_REQUIRE(ctx, gamma, GSS_ERR_INVALID, "%s: gamma_dev is NULL", what);
    GSS_REQUIRE(ctx, scores, GSS_ERR_INVALID, "%s: scores_dev is NULL", what);
    GSS_REQUIRE(ctx, F >= 1, GSS_ERR_INVALID, "%s: F=%d is smaller than 1", what, F);
    GSS_REQUIRE(ctx, T >= 1, GSS_ERR_INVALID, "%s: T=%lld is smaller than 1", what, (long long)T);
    GSS_TRY(check_activity_sizes(ctx, K, D, what));
    GSS_TRY(arena_reserve(ctx, pact_workspace_bytes(F, T, K)));
    return pact_run(ctx, reinterpret_cast<const cplx *>(Y), gamma, F, K, T, D, freq_weights,
                    scores, power);
}

extern "C" int gss_selftest_mfma(gss_ctx *ctx) {
    GSS_ENTER(ctx);
    return selftest_mfma_run(ctx);
}

// ------------------------------------------------------------------ fused pipeline
static int check_params(gss_ctx *ctx, const gss_params *p) {
    GSS_REQUIRE(ctx, p, GSS_ERR_INVALID, "params is NULL");
    GSS_REQUIRE(ctx, p->stft_size == ctx->stft_size && p->stft_shift == ctx->stft_shift,
                GSS_ERR_INVALID, "params stft %d/%d differ from gss_set_windows() %d/%d",
                p->stft_size, p->stft_shift, ctx->stft_size, ctx->stft_shift);
    GSS_REQUIRE(ctx, p->bf >= 0 && p->bf <= 3, GSS_ERR_UNSUPPORTED, "bf=%d", p->bf);
    GSS_REQUIRE(ctx, p->postfilter >= 0 && p->postfilter <= 1, GSS_ERR_UNSUPPORTED,
                "postfilter=%d", p->postfilter);
    GSS_REQUIRE(ctx, p->wpe_psd_context >= 0, GSS_ERR_INVALID, "wpe_psd_context=%d",
                p->wpe_psd_context);
    return GSS_OK;
}

// Arrays of the WPE stage: 0 and 1 = one joint WPE over all D channels; A > 1 = A independent
// WPEs of D / A channels each (gss_params.wpe_arrays)
static int wpe_arrays_of(const gss_params *p) { return p->wpe_arrays > 1 ? p->wpe_arrays : 1; }

static int check_wpe_arrays(gss_ctx *ctx, const gss_params *p, int D) {
    GSS_REQUIRE(ctx, p->wpe_arrays >= 0 && D % wpe_arrays_of(p) == 0, GSS_ERR_INVALID,
                "wpe_arrays=%d does not divide the %d channels into arrays of equal size",
                p->wpe_arrays, D);
    return GSS_OK;
}

// The WPE stage of the pipeline on Fv (virtual) bins of Dv channels, Y -> X.  After
// gss_set_utterances_in_flight(ctx, 1) it runs as two sets of bins side by side on the
// context's stream and its internal second stream -- one set's solve (a chain of latency-bound
// launches, MFMA busy 0.3) under the other's correlation.  Bins are independent: the same bits.
// Measured +1.1 ... +2.1 % at 4 / 12 / 20 / 24 channels for a single utterance and -1.6 %
// when two utterances are in flight anyway (EXPERIMENTS round 6, item 8), hence the hint;
// not the default because overlapped launches no longer have durations of their own (the
// per-kernel table and the roofline of a profile are taken on one stream).  GSS_VARIANT
// wpe_halves=0 / 1 forces it off / on, wpe_halves=n (n > 1) puts 8 n bins into the first set.
static int pipeline_wpe(gss_ctx *ctx, const gss_params *p, const cplx *Y, int Fv, int64_t T,
                        int Dv, cplx *X) {
    const int array_bins = wpe_arrays_of(p) > 1 ? Fv : 0;
    const int halves = gss_variant("wpe_halves", ctx->utterances_in_flight == 1 ? 1 : 0);
    if (!(halves > 0 && Fv >= 32 && p->wpe_iterations > 0))
        return wpe_run(ctx, Y, Fv, T, Dv, p->wpe_taps, p->wpe_delay, p->wpe_iterations,
                       p->wpe_psd_context, X, -1, array_bins);
    GSS_TRY(aux_stream_ready(ctx));
    hipStream_t const main_stream = ctx->stream;
    const int F0 = halves > 1 ? std::min(halves * 8, Fv - 8) : (Fv / 2 + 7) / 8 * 8, F1 = Fv - F0;
    const size_t off = (size_t)F0 * T * Dv;
    int st = wpe_run(ctx, Y, F0, T, Dv, p->wpe_taps, p->wpe_delay, p->wpe_iterations,
                     p->wpe_psd_context, X, 0, array_bins);
    if (st == GSS_OK) {
        GSS_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->aux_stream, ctx->ev_fork, 0));
        ctx->stream = ctx->aux_stream;
        st = wpe_run(ctx, Y + off, F1, T, Dv, p->wpe_taps, p->wpe_delay, p->wpe_iterations,
                     p->wpe_psd_context, X + off, 1, array_bins);
        ctx->stream = main_stream;
        // (joined even when the second part failed to enqueue: nothing may be left running
        // on the internal stream when the call returns)
        GSS_HIP_CHECK(ctx, hipEventRecord(ctx->ev_join, ctx->aux_stream));
        GSS_HIP_CHECK(ctx, hipStreamWaitEvent(main_stream, ctx->ev_join, 0));
    }
    GSS_TRY(st);
    return wpe_copy_zero_pivots(ctx);
}

// The largest stage workspace the pipeline's front (STFT, WPE, activity, EM) needs on top of
// the pipeline's buffers.
static size_t front_stage_bytes(const gss_params *p, int F, int64_t T, int D, int K,
                                bool shared_prior = false) {
    const int A = wpe_arrays_of(p);
    size_t stage = 0;
    // (per-array WPE: R is F A (C taps)^2, C = D / A)
    if (p->wpe)
        stage = std::max(stage, wpe_workspace_bytes(F * A, T, D / A, p->wpe_taps, p->wpe_delay) + (1 << 16));
    // (the shared prior: the reserve of gss_cacgmm_shared_prior)
    stage = std::max(stage, shared_prior ? cacgmm_workspace_bytes(F, T, D, K, /*one_block=*/true) +
                                               cacgmm_prior_workspace_bytes(F, T, K)
                                         : cacgmm_workspace_bytes(F, T, D, K));
    return stage;
}

// What gss_enhance_observation_activity adds to the call: the posterior activity of the
// pipeline's own X and gamma (weights (F,) or NULL, scores (K,T), power (T) or NULL).
struct PipelineActivity {
    const double *weights = nullptr;
    double *scores = nullptr, *power = nullptr;     // scores == NULL: no posterior activity
};

// What an entry point adds to the plain one-target call on float64 samples
// (gss_enhance_observation); each entry fills its own field.  `guided` / `select` say what kind
// of call it is, apart from the descriptor, so that a NULL descriptor is reported and not taken
// for a plain call.
struct PipelineCall {
    const char *entry = "gss_enhance_observation";   // the name in the messages
    int obs_type = 0;                                // samples of obs: 0 = float64, 1 = int16 PCM
    bool guided = false;
    const gss_guidance *guidance = nullptr;
    bool select = false;
    const gss_channel_select *sel = nullptr;
    const gss_bf_segments *seg = nullptr;            // the segment-wise beamformer
    const gss_bf_lcmv *lcmv = nullptr;               // the interferer-nulling beamformer
    const gss_bf_wpd *wpd = nullptr;                 // the WPD beamformer
    const gss_wpe_online_cfg *wpe_online = nullptr;  // the online WPE in the place of the offline one
    const gss_bf_online *bf_online = nullptr;        // the online MVDR in the place of the whole-window one
    const gss_em_online *em_online = nullptr;        // the online CACGMM in the place of the guided EM
    PipelineActivity activity;
    // gss_separate_observation: the EM is the one with a frequency-shared prior, started from
    // this (K,T) table with no mask, in the place of the activity-guided one
    const double *blind_init = nullptr;
    double *blind_prior = nullptr;                   // (K,T), receives the prior of the last M-step
};

// The pipeline's buffers that outlive the front, taken first from the reserved arena; every
// stage runs above them and is released after it.  S > 1 (the targets and the separate calls):
// masks, Xhat and ref in S consecutive per-target blocks.
struct PipelineBuffers {
    cplx *Y, *X;        // the STFT and the WPE output; no WPE: X is Y
    uint8_t *actf;
    double *gamma;
    // WPD: the raw STFT beside the WPE output -- the joint WPE leaves it in Y's buffer, the
    // per-array WPE overwrites that one, hence a copy -- and the frame gate
    cplx *Yraw;
    uint8_t *gate;
    double *mx, *mn;    // (S,F,T) target and distortion masks
    double *mi, *mnn;   // LCMV: the interferer and noise masks (mn = their sum)
    cplx *Xhat;         // (S,T,F)
    int32_t *ref;       // (4 S)
};
static PipelineBuffers pipeline_blocks(Workspace &ws, const gss_params *p, int F, int64_t T,
                                       int64_t T_act, int D, int K, int S, const PipelineCall &call) {
    const size_t ft = (size_t)F * T;
    PipelineBuffers b;
    b.Y = ws.take<cplx>(ft * D, "pipeline Y");
    b.X = p->wpe ? ws.take<cplx>(ft * D, "pipeline X") : b.Y;
    b.actf = ws.take<uint8_t>((size_t)K * T_act, "pipeline frame activity");
    b.gamma = ws.take<double>(ft * K, "pipeline gamma");
    const bool raw_copy = call.wpd && p->wpe && wpe_arrays_of(p) > 1;
    b.Yraw = raw_copy ? ws.take<cplx>(ft * D, "pipeline raw Y") : nullptr;
    b.gate = call.wpd ? ws.take<uint8_t>((size_t)T, "pipeline frame gate") : nullptr;
    b.mx = ws.take<double>(S * ft, "pipeline target mask");
    b.mn = ws.take<double>(S * ft, "pipeline distortion mask");
    b.mi = call.lcmv ? ws.take<double>(ft, "pipeline interferer mask") : nullptr;
    b.mnn = call.lcmv ? ws.take<double>(ft, "pipeline noise mask") : nullptr;
    b.Xhat = ws.take<cplx>(S * ft, "pipeline Xhat");
    b.ref = ws.take<int32_t>(4 * (size_t)S, "pipeline ref");
    return b;
}
// Single blocks above the pipeline's buffers: the STFT of all D_all channels until the kept ones
// are gathered (a selection), the one channel-picked X_hat of a targets call ('ch2' / 'sum'), the
// scores of the separate call's posterior activity, which nobody asked for
static cplx *select_all_blocks(Workspace &ws, int F, int64_t T, int D_all) {
    return ws.take<cplx>((size_t)F * T * D_all, "pipeline Y of all channels");
}
static cplx *channel_pick_blocks(Workspace &ws, int F, int64_t T) {
    return ws.take<cplx>((size_t)F * T, "pipeline picked channel");
}
static double *separate_scores_blocks(Workspace &ws, int K, int64_t T) {
    return ws.take<double>((size_t)K * T, "separate scores");
}

// The reserve of the one-target call: its buffers and the largest stage above them.
// (seg: the segment-wise beamformer in the place of the whole-window one;
// select: D is the number of channels kept out of D_all, and the selection stage needs its own
// workspace and, when it gathers, the STFT of all D_all channels;
// activity: the posterior activity runs between the front and the masks)
static size_t pipeline_workspace(const gss_params *p, int F, int64_t T, int64_t T_act, int D,
                                 int K, int D_all, const PipelineCall &call) {
    const gss_bf_wpd *const wpd = call.wpd;
    const bool lcmv = call.lcmv != nullptr;
    Workspace ws, all;
    pipeline_blocks(ws, p, F, T, T_act, D, K, 1, call);
    if (D_all > D) select_all_blocks(all, F, T, D_all);
    size_t stage = front_stage_bytes(p, F, T, D, K);
    stage = std::max(stage, call.seg
                                ? mvdr_segments_workspace_bytes(F, T, D, call.seg->segment_frames)
                                : mvdr_workspace_bytes(F, T, D));
    if (lcmv)
        stage = std::max(stage, std::max(lcmv_workspace_bytes(F, T, D),
                                         lcmv_masks_workspace_bytes(F, K)));
    if (wpd) stage = std::max(stage, wpd_workspace_bytes(F, T, D, wpd->taps, wpd->delay));
    // (online WPE from a fresh state: F A (n^2 + n C + L C) complex values of state -- the joint
    // 24-channel case, n = 240, is the large one -- and sigma)
    if (call.wpe_online && p->wpe)
        stage = std::max(stage, wpe_online_workspace_bytes(F, T, wpe_arrays_of(p), D / wpe_arrays_of(p),
                                                           p->wpe_taps, p->wpe_delay, true));
    // (online MVDR: the state of a fresh call, and the whole-window pass that picks the channel)
    if (call.bf_online)
        stage = std::max(stage, mvdr_online_workspace_bytes(F, T, D, true, call.bf_online->ref_channel < 0));
    if (call.em_online) stage = std::max(stage, cacgmm_online_workspace_bytes(F, K, D, true));
    stage = std::max(stage, stft_workspace_bytes(T, p->stft_size));
    if (call.activity.scores)
        stage = std::max(stage, pact_workspace_bytes(F, T, K));   // the partial planes
    if (call.select)
        stage = std::max(stage, chsel_workspace_bytes(F, T, D_all, call.sel->bands) + all.bytes + 4096);
    return ws.bytes + 4096 + stage + (1 << 16);
}

// The same with the tail of S targets: masks, Xhat and the beamformer's intermediates S times,
// S iSTFT frame buffers, one channel-picked X_hat ('ch2' / 'sum').  blind
// (gss_separate_observation, S = K): the EM with the shared prior in the place of the guided
// one, and the posterior activity's partial planes and scores.
static size_t targets_workspace(const gss_params *p, int F, int64_t T, int64_t T_act, int D,
                                int K, int S, bool blind) {
    Workspace ws, scores, picked;
    pipeline_blocks(ws, p, F, T, T_act, D, K, S, PipelineCall{});
    separate_scores_blocks(scores, K, T);
    channel_pick_blocks(picked, F, T);
    size_t stage = front_stage_bytes(p, F, T, D, K, /*shared_prior=*/blind);
    if (blind) stage = std::max(stage, pact_workspace_bytes(F, T, K) + scores.bytes + 4096);
    stage = std::max(stage, mvdr_workspace_bytes(F, T, D, S));
    stage = std::max(stage, picked.bytes + 4096);
    stage = std::max(stage, stft_workspace_bytes((int64_t)S * T, p->stft_size));
    return ws.bytes + 4096 + stage + (1 << 16);
}

// Checks of the fused pipeline that do not depend on the target(s): before ...
static int check_pipeline_front(gss_ctx *ctx, const gss_params *p, const void *obs, int D,
                                int64_t N, const void *act, const void *out, const char *what) {
    GSS_TRY(check_windows(ctx));
    GSS_TRY(check_params(ctx, p));
    // (`act`: the time-domain activity, or the descriptor of a guided call)
    GSS_REQUIRE(ctx, obs && act && out && N >= 1, GSS_ERR_INVALID, "%s: bad arguments", what);
    GSS_REQUIRE(ctx, D >= 1 && D <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED, "D=%d", D);
    return GSS_OK;
}

// ... and after those of the targets; the frame counts T, T_act of the window.
static int check_pipeline_rest(gss_ctx *ctx, const gss_params *p, int D, int64_t N, int K,
                               int64_t N_act, int64_t *T_out, int64_t *T_act_out) {
    GSS_TRY(check_cacgmm_args(ctx, D, K, p->bss_iterations, p->bss_iterations_post));
    if (p->wpe) GSS_TRY(check_wpe_arrays(ctx, p, D));   // (no WPE: the field is not read)
    if (p->bf == 0 || p->bf == 3) GSS_TRY(check_bf_channels(ctx, D));
    if (p->bf == 1)
        GSS_REQUIRE(ctx, D > 2, GSS_ERR_INVALID, "bf='ch2' needs more than 2 channels");

    const int size = p->stft_size, shift = p->stft_shift, fading = p->stft_fading;
    const int F = size / 2 + 1;
    const int64_t T = gss_stft_num_frames(N, size, shift, fading);
    const int64_t T_act = gss_stft_num_frames(N_act, size, shift, fading);
    // GSS.__call__ uses initialization[..., :T]: fewer activity frames than STFT
    // frames is a shape error in the reference too
    GSS_REQUIRE(ctx, T_act >= T, GSS_ERR_INVALID,
                "activity covers %lld frames but the observation has %lld",
                (long long)T_act, (long long)T);

    GSS_TRY(check_stft_bins(ctx, F, T, D));
    *T_out = T;
    *T_act_out = T_act;
    return GSS_OK;
}

// STFT, WPE (joint or per array), frame activity and the guided CACGMM of one window: obs ->
// X (F,T,D) and gamma (F,K,T), nothing of it depending on a target.  Stage workspace above
// `mark` is released after each stage.  `guide` (a guided call): the model's guidance per STFT
// frame as the caller gives it, instead of the frame activity made from `act`.  `D_all` (a
// selection): the channels of `obs`, of which D are kept.
static int run_front(gss_ctx *ctx, const gss_params *p, const PipelineCall &call, const void *obs,
                     int D_all, int D, int64_t N, const uint8_t *act, int K, int64_t N_act, int F,
                     int64_t T, int64_t T_act, const PipelineBuffers &fr, size_t mark,
                     const EmGuide &guide) {
    const int obs_type = call.obs_type;
    cplx *const Y = fr.Y, *const X = fr.X;
    if (!call.select) {
        GSS_TRY(stft_run(ctx, obs, obs_type, D, N, p->stft_fading, Y));
    } else if (D == D_all) {
        // every channel is kept: ranked (the status words name them), nothing moves
        GSS_TRY(stft_run(ctx, obs, obs_type, D, N, p->stft_fading, Y));
        GSS_TRY(chsel_select_run(ctx, Y, F, T, D, *call.sel, nullptr, nullptr));
        GSS_TRY(arena_release(ctx, mark));
    } else {
        // the STFT of all D_all channels lives above `mark` until the kept D = sel->keep of
        // them are gathered into Y
        Workspace ws(ctx);
        cplx *Yall = select_all_blocks(ws, F, T, D_all);
        GSS_TRY(ws.status(call.entry));
        GSS_TRY(stft_run(ctx, obs, obs_type, D_all, N, p->stft_fading, Yall));
        GSS_TRY(chsel_select_run(ctx, Yall, F, T, D_all, *call.sel, Y, nullptr));
        GSS_TRY(arena_release(ctx, mark));
    }
    if (fr.Yraw)
        GSS_HIP_CHECK(ctx, hipMemcpyAsync(fr.Yraw, Y, sizeof(cplx) * (size_t)F * T * D,
                                          hipMemcpyDeviceToDevice, ctx->stream));
    if (!p->wpe)    // no solve in this call: clear the count an earlier utterance left behind
        GSS_HIP_CHECK(ctx, hipMemsetAsync(ctx->status_dev + GSS_STATUS_WPE_ZERO_PIVOTS, 0,
                                          sizeof(int32_t), ctx->stream));
    const int A = wpe_arrays_of(p);
    if (p->wpe && call.wpe_online) {
        // the online WPE reads the array-major channels where they are: no regrouping; no solve,
        // so the pivot count an earlier utterance left behind is cleared
        GSS_HIP_CHECK(ctx, hipMemsetAsync(ctx->status_dev + GSS_STATUS_WPE_ZERO_PIVOTS, 0,
                                          sizeof(int32_t), ctx->stream));
        GSS_TRY(wpe_online_run(ctx, Y, F, T, A, D / A, p->wpe_taps, p->wpe_delay,
                               call.wpe_online->alpha, nullptr, nullptr, nullptr, X,
                               gss_variant_set("wpe_online_mem")));
        GSS_TRY(arena_release(ctx, mark));
    } else if (p->wpe && A == 1) {
        GSS_TRY(pipeline_wpe(ctx, p, Y, F, T, D, X));
        GSS_TRY(arena_release(ctx, mark));
    } else if (p->wpe) {
        // per-array WPE: Y (F, T, A C) is regrouped into X's buffer as (F A, T, C), WPE writes
        // (F A, T, C) into Y's buffer (Y is not read after this stage), and that is scattered
        // back into X as (F, T, A C) for GSS and the beamformer
        GSS_TRY(wpe_arrays_regroup_run(ctx, Y, F, T, A, D / A, true, X));
        GSS_TRY(pipeline_wpe(ctx, p, X, F * A, T, D / A, Y));
        GSS_TRY(wpe_arrays_regroup_run(ctx, Y, F, T, A, D / A, false, X));
        GSS_TRY(arena_release(ctx, mark));
    }
    if (call.blind_init) {
        // gss_cacgmm_shared_prior(init, no mask, bss_iterations, post = 1): fit, then predict
        EmSchedule s;
        s.iterations = p->bss_iterations;
        s.gamma = fr.gamma;
        s.shared_prior = true;
        s.prior = call.blind_prior;
        GSS_TRY(cacgmm_schedule_run(ctx, X, F, T, D, EmGuide{call.blind_init, nullptr, 0, T, 0, 0},
                                    K, s));
        GSS_TRY(arena_release(ctx, mark));
        return GSS_OK;
    }
    if (!call.guided) GSS_TRY(activity_run(ctx, act, K, N_act, p->stft_fading, fr.actf));
    if (call.em_online) {   // (never guided, checked by the entry point)
        GSS_TRY(cacgmm_online_run(ctx, X, F, T, D, em_guide_from_activity(fr.actf, T_act), K,
                                  call.em_online->forget, call.em_online->prior_mass, nullptr, nullptr,
                                  fr.gamma));
        GSS_TRY(arena_release(ctx, mark));
        return GSS_OK;
    }
    GSS_TRY(cacgmm_run(ctx, X, F, T, D, call.guided ? guide : em_guide_from_activity(fr.actf, T_act),
                       K, p->bss_iterations, p->bss_iterations_post, fr.gamma));
    GSS_TRY(arena_release(ctx, mark));
    return GSS_OK;
}

static int copy_tap(gss_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!dst) return GSS_OK;
    GSS_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return GSS_OK;
}

// The front's debug taps: Obs_ftd, act_frames, gamma
static int copy_front_taps(gss_ctx *ctx, const gss_debug_taps *taps, const PipelineBuffers &fr,
                           int F, int64_t T, int64_t T_act, int D, int K) {
    GSS_TRY(copy_tap(ctx, taps->Obs_ftd, fr.X, sizeof(cplx) * (size_t)F * T * D));
    if (taps->act_frames)
        GSS_HIP_CHECK(ctx, hipMemcpy2DAsync(taps->act_frames, (size_t)T, fr.actf, (size_t)T_act,
                                            (size_t)T, (size_t)K, hipMemcpyDeviceToDevice,
                                            ctx->stream));
    GSS_TRY(copy_tap(ctx, taps->gamma, fr.gamma, sizeof(double) * (size_t)F * K * T));
    return GSS_OK;
}

static int enhance_observation_impl(gss_ctx *ctx, const gss_params *p, const void *obs, int D,
                                    int64_t N, const uint8_t *act, int K, int64_t N_act,
                                    int target, int64_t start_ctx, int64_t end_ctx, double *out,
                                    const gss_debug_taps *taps, const PipelineCall &call) {
    GSS_REQUIRE(ctx, !call.guided || call.guidance, GSS_ERR_INVALID,
                "gss_enhance_observation_guided: guidance is NULL");
    GSS_TRY(check_pipeline_front(ctx, p, obs, D, N,
                                 call.guided ? (const void *)call.guidance : act, out, call.entry));
    // a selection: D_all channels come in, the pipeline below runs on the D = sel->keep kept
    const int D_all = D;
    if (call.select) {
        GSS_TRY(check_channel_select(ctx, call.sel, D, true, "gss_enhance_observation_select"));
        GSS_REQUIRE(ctx, !(p->wpe && p->wpe_arrays > 1), GSS_ERR_UNSUPPORTED,
                    "gss_enhance_observation_select: wpe_arrays=%d, a selection breaks the equal "
                    "arrays of the per-array WPE", p->wpe_arrays);
        GSS_REQUIRE(ctx, p->bf != 1, GSS_ERR_UNSUPPORTED,
                    "gss_enhance_observation_select: bf=1 ('ch2') names a physical channel");
        const int64_t T_all = gss_stft_num_frames(N, p->stft_size, p->stft_shift, p->stft_fading);
        GSS_TRY(check_stft_bins(ctx, p->stft_size / 2 + 1, T_all, D_all));
        D = call.sel->keep;
    }
    GSS_REQUIRE(ctx, !call.guided || !taps || !taps->act_frames, GSS_ERR_INVALID,
                "gss_enhance_observation_guided: taps->act_frames must be NULL (a guided call "
                "has no frame activity)");
    GSS_TRY(check_target_index(ctx, target, K));
    // core.py:221-222
    GSS_REQUIRE(ctx, start_ctx >= 0 && end_ctx >= 0, GSS_ERR_INVALID,
                "assert context samples >= 0 failed: %lld %lld", (long long)start_ctx,
                (long long)end_ctx);
    int64_t T, T_act;
    GSS_TRY(check_pipeline_rest(ctx, p, D, N, K, N_act, &T, &T_act));
    const int size = p->stft_size, shift = p->stft_shift, fading = p->stft_fading;
    const int F = size / 2 + 1;
    EmGuide guide{};
    if (call.guided) GSS_TRY(check_guidance(ctx, call.guidance, K, T, &guide));

    GSS_TRY(arena_reserve(ctx, pipeline_workspace(p, F, T, T_act, D, K, D_all, call)));
    Workspace ws(ctx);
    const PipelineBuffers fr = pipeline_blocks(ws, p, F, T, T_act, D, K, 1, call);
    GSS_TRY(ws.status(call.entry));
    uint8_t *const gate = fr.gate;
    double *const mx = fr.mx, *const mn = fr.mn, *const mi = fr.mi, *const mnn = fr.mnn;
    cplx *const Xhat = fr.Xhat;
    int32_t *const ref = fr.ref;
    const size_t mark = ctx->arena_off;
    GSS_TRY(run_front(ctx, p, call, obs, D_all, D, N, act, K, N_act, F, T, T_act, fr, mark, guide));
    cplx *const X = fr.X;
    if (call.activity.scores) {      // (reads X and gamma, writes the caller's buffers only)
        GSS_TRY(pact_run(ctx, X, fr.gamma, F, K, T, D, call.activity.weights,
                         call.activity.scores, call.activity.power));
        GSS_TRY(arena_release(ctx, mark));
    }

    int64_t sf = 0, ef = 0;
    if (p->bf_drop_context) {
        sf = gss_samples_to_stft_frames(start_ctx, size, shift, fading);
        ef = gss_samples_to_stft_frames(end_ctx, size, shift, fading);
    }
    // (the LCMV takes its three masks below; mx, mn are the taps' masks there: the target and
    // I + N, the sum over the other classes)
    if (!call.lcmv || (taps && taps->distortion_mask))
        GSS_TRY(masks_from_posteriors_run(ctx, fr.gamma, F, K, T, target, p->bf_drop_context, sf,
                                          ef, mx, mn));
    if (call.wpd) {     // (bf == 0, checked by the entry point) on the STFT before WPE
        const cplx *raw = fr.Yraw ? fr.Yraw : fr.Y;
        if (p->bf_drop_context) GSS_TRY(wpd_context_gate_run(ctx, T, sf, ef, gate));
        GSS_TRY(wpd_run(ctx, raw, F, T, D, mx, p->bf_drop_context ? gate : nullptr, *call.wpd,
                        /*forced_ref=*/-1, Xhat, ref));
        GSS_TRY(arena_release(ctx, mark));
    } else if (call.lcmv) {   // (bf == 0, checked by the entry point)
        GSS_TRY(lcmv_masks_run(ctx, fr.gamma, F, K, T, target, *call.lcmv, p->bf_drop_context, sf, ef,
                               mx, mi, mnn, nullptr));
        GSS_TRY(arena_release(ctx, mark));
        GSS_TRY(lcmv_run(ctx, X, F, T, D, mx, mi, mnn, /*ban=*/1, /*forced_ref=*/-1,
                         call.lcmv->min_mass, Xhat, ref));
        GSS_TRY(arena_release(ctx, mark));
    } else if (call.bf_online) {   // (bf == 0, checked by the entry point); Xhat is (T,F)
        GSS_TRY(mvdr_online_run(ctx, X, F, T, D, mx, mn, /*ban=*/1, call.bf_online->forget,
                                call.bf_online->loading, call.bf_online->ref_channel, nullptr, nullptr,
                                Xhat, 1, F, nullptr, ref));
        GSS_TRY(arena_release(ctx, mark));
    } else if (call.seg) {   // (bf == 0, checked by the entry point)
        GSS_TRY(mvdr_segments_run(ctx, X, F, T, D, mx, mn, /*ban=*/1, *call.seg, Xhat, ref));
        GSS_TRY(arena_release(ctx, mark));
    } else if (p->bf == 0 || p->bf == 3) {
        GSS_TRY(mvdr_run(ctx, X, F, T, D, mx, mn, /*ban=*/1, Xhat, ref, /*gev=*/p->bf == 3));
        GSS_TRY(arena_release(ctx, mark));
    } else {
        GSS_TRY(channel_pick_run(ctx, X, F, T, D, p->bf, Xhat));
    }
    if (p->postfilter == 1) GSS_TRY(mask_mul_run(ctx, Xhat, mx, F, T));
    GSS_TRY(istft_run(ctx, Xhat, T, fading, out));

    if (taps) {
        GSS_TRY(copy_front_taps(ctx, taps, fr, F, T, T_act, D, K));
        GSS_TRY(copy_tap(ctx, taps->target_mask, mx, sizeof(double) * (size_t)F * T));
        GSS_TRY(copy_tap(ctx, taps->distortion_mask, mn, sizeof(double) * (size_t)F * T));
        GSS_TRY(copy_tap(ctx, taps->Xhat, Xhat, sizeof(cplx) * (size_t)F * T));
        if (p->bf == 0 || p->bf == 3) GSS_TRY(copy_tap(ctx, taps->ref_channel, ref, sizeof(int32_t)));
    }
    return GSS_OK;
}

// The target-dependent tail for S targets together (masks, beamformer or channel pick,
// postfilter, iSTFT, the taps) on the front's X and gamma; start_ctx / end_ctx NULL: no context
// frames.  The buffers of `fr`, everything below `mark`, stay allocated.
static int run_targets_tail(gss_ctx *ctx, const gss_params *p, const PipelineBuffers &fr, int F,
                            int64_t T, int64_t T_act, int D, int K, int S, const int32_t *targets,
                            const int64_t *start_ctx, const int64_t *end_ctx, size_t mark,
                            double *out, const gss_debug_taps *taps) {
    const int size = p->stft_size, shift = p->stft_shift, fading = p->stft_fading;
    cplx *const X = fr.X, *const Xhat = fr.Xhat;
    double *const mx = fr.mx, *const mn = fr.mn;
    int32_t *const ref = fr.ref;
    int64_t sf[GSS_MAX_CLASSES] = {}, ef[GSS_MAX_CLASSES] = {};
    if (p->bf_drop_context && start_ctx && end_ctx) {
        for (int s = 0; s < S; ++s) {
            sf[s] = gss_samples_to_stft_frames(start_ctx[s], size, shift, fading);
            ef[s] = gss_samples_to_stft_frames(end_ctx[s], size, shift, fading);
        }
    }
    GSS_TRY(masks_targets_run(ctx, fr.gamma, F, K, T, S, targets, p->bf_drop_context, sf, ef, mx,
                              mn));
    const bool beamformer = p->bf == 0 || p->bf == 3;
    if (beamformer) {
        GSS_TRY(mvdr_run(ctx, X, F, T, D, mx, mn, /*ban=*/1, Xhat, ref, /*gev=*/p->bf == 3,
                         /*forced_ref=*/-1, S, /*targets=*/true));
        GSS_TRY(arena_release(ctx, mark));
        if (p->postfilter == 1)
            GSS_TRY(mask_mul_targets_run(ctx, Xhat, (int64_t)F * T, Xhat, mx, F, T, S, 1));
    } else {
        // 'ch2' / 'sum' do not depend on the target: one X_hat, then each target's copy of it
        // (times its mask with the postfilter)
        Workspace ws(ctx);
        cplx *X1 = channel_pick_blocks(ws, F, T);
        GSS_TRY(ws.status("channel pick of a targets call"));
        GSS_TRY(channel_pick_run(ctx, X, F, T, D, p->bf, X1));
        GSS_TRY(mask_mul_targets_run(ctx, X1, 0, Xhat, mx, F, T, S, p->postfilter == 1));
        GSS_TRY(arena_release(ctx, mark));
    }
    GSS_TRY(istft_run(ctx, Xhat, T, fading, out, S));

    if (taps) {
        GSS_TRY(copy_front_taps(ctx, taps, fr, F, T, T_act, D, K));
        GSS_TRY(copy_tap(ctx, taps->target_mask, mx, sizeof(double) * (size_t)S * F * T));
        GSS_TRY(copy_tap(ctx, taps->distortion_mask, mn, sizeof(double) * (size_t)S * F * T));
        GSS_TRY(copy_tap(ctx, taps->Xhat, Xhat, sizeof(cplx) * (size_t)S * F * T));
        if (beamformer && taps->ref_channel)
            GSS_HIP_CHECK(ctx, hipMemcpyAsync(taps->ref_channel, ref, sizeof(int32_t) * S,
                                              hipMemcpyDeviceToDevice, ctx->stream));
    }
    return GSS_OK;
}

// S targets of one window: the front once, then the target-dependent tail for all S targets
// together -- masks, PSD, solve, reference channel, apply, postfilter and iSTFT each one launch
// over S per-target blocks.  Row s of `out` and of every per-target tap is what
// enhance_observation_impl gives for target_index[s] with that target's contexts.
static int enhance_observation_targets_impl(gss_ctx *ctx, const gss_params *p, const void *obs,
                                            int obs_type, int D, int64_t N, const uint8_t *act,
                                            int K, int64_t N_act, int S, const int32_t *targets,
                                            const int64_t *start_ctx, const int64_t *end_ctx,
                                            double *out, const gss_debug_taps *taps) {
    // (the status words of this call: none until its beamformer runs -- a call that fails before
    // it, or a 'ch2' / 'sum' call, leaves no per-target words behind)
    ctx->last_targets = 0;
    GSS_TRY(check_pipeline_front(ctx, p, obs, D, N, act, out, "gss_enhance_observation_targets"));
    GSS_REQUIRE(ctx, targets && start_ctx && end_ctx, GSS_ERR_INVALID,
                "gss_enhance_observation_targets: NULL target or context array");
    // (K bounded before the indices are used as bit positions below)
    GSS_TRY(check_class_count(ctx, K));
    GSS_REQUIRE(ctx, S >= 1 && S <= K, GSS_ERR_INVALID,
                "%d targets of %d classes: need 1 <= S <= K", S, K);
    uint32_t seen = 0;
    for (int s = 0; s < S; ++s) {
        GSS_REQUIRE(ctx, targets[s] >= 0 && targets[s] < K, GSS_ERR_INVALID,
                    "target_index[%d] = %d outside [0, %d)", s, targets[s], K);
        GSS_REQUIRE(ctx, !(seen >> targets[s] & 1u), GSS_ERR_INVALID,
                    "target_index[%d] = %d is given twice", s, targets[s]);
        seen |= 1u << targets[s];
        GSS_REQUIRE(ctx, start_ctx[s] >= 0 && end_ctx[s] >= 0, GSS_ERR_INVALID,
                    "assert context samples >= 0 failed: %lld %lld (target %d)",
                    (long long)start_ctx[s], (long long)end_ctx[s], s);
    }
    int64_t T, T_act;
    GSS_TRY(check_pipeline_rest(ctx, p, D, N, K, N_act, &T, &T_act));
    const int F = p->stft_size / 2 + 1;

    PipelineCall call;
    call.obs_type = obs_type;
    GSS_TRY(arena_reserve(ctx, targets_workspace(p, F, T, T_act, D, K, S, /*blind=*/false)));
    Workspace ws(ctx);
    const PipelineBuffers fr = pipeline_blocks(ws, p, F, T, T_act, D, K, S, call);
    GSS_TRY(ws.status("gss_enhance_observation_targets"));
    const size_t mark = ctx->arena_off;
    GSS_TRY(run_front(ctx, p, call, obs, D, D, N, act, K, N_act, F, T, T_act, fr, mark, EmGuide{}));
    return run_targets_tail(ctx, p, fr, F, T, T_act, D, K, S, targets, start_ctx, end_ctx, mark, out,
                            taps);
}

extern "C" int gss_enhance_observation(gss_ctx *ctx, const gss_params *p, const double *obs,
                                       int D, int64_t N, const uint8_t *act, int K,
                                       int64_t N_act, int target, int64_t start_ctx,
                                       int64_t end_ctx, double *out,
                                       const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    return enhance_observation_impl(ctx, p, obs, D, N, act, K, N_act, target, start_ctx, end_ctx,
                                    out, taps, PipelineCall{});
}

extern "C" int gss_enhance_observation_guided(gss_ctx *ctx, const gss_params *p,
                                              const double *obs, int D, int64_t N,
                                              const gss_guidance *guidance, int K, int target,
                                              int64_t start_ctx, int64_t end_ctx, double *out,
                                              const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    // (the frame counts of observation and guidance are one: N_act = N)
    PipelineCall call;
    call.entry = "gss_enhance_observation_guided";
    call.guided = true;
    call.guidance = guidance;
    return enhance_observation_impl(ctx, p, obs, D, N, nullptr, K, N, target, start_ctx, end_ctx,
                                    out, taps, call);
}

extern "C" int gss_enhance_observation_segments(gss_ctx *ctx, const gss_params *p,
                                                const double *obs, int D, int64_t N,
                                                const uint8_t *act, int K, int64_t N_act,
                                                int target, int64_t start_ctx, int64_t end_ctx,
                                                const gss_bf_segments *seg, double *out,
                                                const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    GSS_TRY(check_segments(ctx, seg, "gss_enhance_observation_segments"));
    GSS_REQUIRE(ctx, !p || p->bf == 0, GSS_ERR_UNSUPPORTED,
                "gss_enhance_observation_segments: bf=%d, only 0 ('mvdrSouden_ban') has segments",
                p->bf);
    PipelineCall call;
    call.seg = seg;
    return enhance_observation_impl(ctx, p, obs, D, N, act, K, N_act, target, start_ctx, end_ctx,
                                    out, taps, call);
}

extern "C" int gss_enhance_observation_wpd(gss_ctx *ctx, const gss_params *p, const double *obs,
                                           int D, int64_t N, const uint8_t *act, int K,
                                           int64_t N_act, int target, int64_t start_ctx,
                                           int64_t end_ctx, const gss_bf_wpd *wpd, double *out,
                                           const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    GSS_REQUIRE(ctx, !p || p->bf == 0, GSS_ERR_UNSUPPORTED,
                "gss_enhance_observation_wpd: bf=%d, only 0 ('mvdrSouden_ban') has a WPD form",
                p->bf);
    GSS_TRY(check_wpd(ctx, wpd, D, "gss_enhance_observation_wpd"));
    PipelineCall call;
    call.wpd = wpd;
    return enhance_observation_impl(ctx, p, obs, D, N, act, K, N_act, target, start_ctx, end_ctx,
                                    out, taps, call);
}

extern "C" int gss_enhance_observation_wpe_online(gss_ctx *ctx, const gss_params *p,
                                                  const double *obs, int D, int64_t N,
                                                  const uint8_t *act, int K, int64_t N_act,
                                                  int target, int64_t start_ctx, int64_t end_ctx,
                                                  const gss_wpe_online_cfg *cfg, double *out,
                                                  const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    const char *const what = "gss_enhance_observation_wpe_online";
    GSS_REQUIRE(ctx, cfg, GSS_ERR_INVALID, "%s: cfg is NULL", what);
    GSS_REQUIRE(ctx, p, GSS_ERR_INVALID, "%s: params is NULL", what);
    GSS_REQUIRE(ctx, p->wpe, GSS_ERR_INVALID, "%s: wpe = 0, there is no WPE stage to replace", what);
    GSS_REQUIRE(ctx, p->wpe_psd_context == 0, GSS_ERR_INVALID,
                "%s: wpe_psd_context = %d, the online WPE has no PSD context", what,
                p->wpe_psd_context);
    GSS_REQUIRE(ctx, D >= 1 && D <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED, "D=%d", D);
    GSS_TRY(check_wpe_arrays(ctx, p, D));
    GSS_TRY(check_wpe_online(ctx, what, 1, wpe_arrays_of(p), D / wpe_arrays_of(p), p->wpe_taps,
                             p->wpe_delay, cfg->alpha));
    PipelineCall call;
    call.entry = what;
    call.wpe_online = cfg;
    return enhance_observation_impl(ctx, p, obs, D, N, act, K, N_act, target, start_ctx, end_ctx,
                                    out, taps, call);
}

// The checks of an online MVDR in a fused call and its fields of the call description
// (wpe_cfg: storage for the online WPE's settings, which must outlive the call).
static int fill_bf_online(gss_ctx *ctx, const char *what, const gss_params *p,
                          const gss_bf_online *cfg, int D, PipelineCall *call,
                          gss_wpe_online_cfg *wpe_cfg) {
    GSS_TRY(check_bf_online(ctx, what, cfg, D));
    GSS_REQUIRE(ctx, p->bf == 0, GSS_ERR_UNSUPPORTED,
                "%s: bf=%d, only 0 ('mvdrSouden_ban') has an online form", what, p->bf);
    call->bf_online = cfg;
    wpe_cfg->alpha = cfg->wpe_alpha;
    if (cfg->wpe_online) {
        GSS_REQUIRE(ctx, p->wpe, GSS_ERR_INVALID, "%s: wpe = 0, there is no WPE stage to replace",
                    what);
        GSS_REQUIRE(ctx, p->wpe_psd_context == 0, GSS_ERR_INVALID,
                    "%s: wpe_psd_context = %d, the online WPE has no PSD context", what,
                    p->wpe_psd_context);
        GSS_TRY(check_wpe_arrays(ctx, p, D));
        GSS_TRY(check_wpe_online(ctx, what, 1, wpe_arrays_of(p), D / wpe_arrays_of(p), p->wpe_taps,
                                 p->wpe_delay, cfg->wpe_alpha));
        call->wpe_online = wpe_cfg;
    }
    return GSS_OK;
}

extern "C" int gss_enhance_observation_bf_online(gss_ctx *ctx, const gss_params *p,
                                                 const double *obs, int D, int64_t N,
                                                 const uint8_t *act, int K, int64_t N_act,
                                                 int target, int64_t start_ctx, int64_t end_ctx,
                                                 const gss_bf_online *cfg, double *out,
                                                 const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    const char *const what = "gss_enhance_observation_bf_online";
    GSS_REQUIRE(ctx, p, GSS_ERR_INVALID, "%s: params is NULL", what);
    PipelineCall call;
    call.entry = what;
    gss_wpe_online_cfg wpe_cfg{};
    GSS_TRY(fill_bf_online(ctx, what, p, cfg, D, &call, &wpe_cfg));
    return enhance_observation_impl(ctx, p, obs, D, N, act, K, N_act, target, start_ctx, end_ctx,
                                    out, taps, call);
}

extern "C" int gss_enhance_observation_gss_online(gss_ctx *ctx, const gss_params *p,
                                                  const double *obs, int D, int64_t N,
                                                  const uint8_t *act, int K, int64_t N_act,
                                                  int target, int64_t start_ctx, int64_t end_ctx,
                                                  const gss_em_online *em, const gss_bf_online *bf,
                                                  double *out, const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    const char *const what = "gss_enhance_observation_gss_online";
    GSS_REQUIRE(ctx, p, GSS_ERR_INVALID, "%s: params is NULL", what);
    GSS_TRY(check_em_online(ctx, what, em));
    GSS_REQUIRE(ctx, K <= GSS_CACGMM_ONLINE_MAX_CLASSES, GSS_ERR_UNSUPPORTED,
                "%s: K = %d is larger than %d", what, K, GSS_CACGMM_ONLINE_MAX_CLASSES);
    PipelineCall call;
    call.entry = what;
    call.em_online = em;
    gss_wpe_online_cfg wpe_cfg{};
    if (bf) GSS_TRY(fill_bf_online(ctx, what, p, bf, D, &call, &wpe_cfg));
    return enhance_observation_impl(ctx, p, obs, D, N, act, K, N_act, target, start_ctx, end_ctx,
                                    out, taps, call);
}

extern "C" int gss_enhance_observation_lcmv(gss_ctx *ctx, const gss_params *p, const double *obs,
                                            int D, int64_t N, const uint8_t *act, int K,
                                            int64_t N_act, int target, int64_t start_ctx,
                                            int64_t end_ctx, const gss_bf_lcmv *lcmv,
                                            double *out, const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    GSS_REQUIRE(ctx, !p || p->bf == 0, GSS_ERR_UNSUPPORTED,
                "gss_enhance_observation_lcmv: bf=%d, only 0 ('mvdrSouden_ban') has an "
                "interferer-nulling form", p->bf);
    GSS_TRY(check_class_count(ctx, K));
    GSS_TRY(check_target_index(ctx, target, K));
    GSS_TRY(check_lcmv(ctx, lcmv, K, target, "gss_enhance_observation_lcmv"));
    GSS_TRY(check_lcmv_channels(ctx, D, "gss_enhance_observation_lcmv"));
    PipelineCall call;
    call.lcmv = lcmv;
    return enhance_observation_impl(ctx, p, obs, D, N, act, K, N_act, target, start_ctx, end_ctx,
                                    out, taps, call);
}

extern "C" int gss_enhance_observation_activity(gss_ctx *ctx, const gss_params *p,
                                                const double *obs, int D, int64_t N,
                                                const uint8_t *act, int K, int64_t N_act,
                                                int target, int64_t start_ctx, int64_t end_ctx,
                                                const double *freq_weights, double *out,
                                                double *scores, double *power,
                                                const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    const char *what = "gss_enhance_observation_activity";
    GSS_REQUIRE(ctx, p, GSS_ERR_INVALID, "%s: params is NULL", what);
    GSS_REQUIRE(ctx, obs, GSS_ERR_INVALID, "%s: obs_dev is NULL", what);
    GSS_REQUIRE(ctx, act, GSS_ERR_INVALID, "%s: act_dev is NULL", what);
    GSS_REQUIRE(ctx, out, GSS_ERR_INVALID, "%s: out_dev is NULL", what);
    GSS_REQUIRE(ctx, scores, GSS_ERR_INVALID, "%s: scores_dev is NULL", what);
    GSS_REQUIRE(ctx, N >= 1, GSS_ERR_INVALID, "%s: N=%lld is smaller than 1", what, (long long)N);
    GSS_TRY(check_activity_sizes(ctx, K, D, what));
    PipelineCall call;
    call.activity.weights = freq_weights;
    call.activity.scores = scores;
    call.activity.power = power;
    return enhance_observation_impl(ctx, p, obs, D, N, act, K, N_act, target, start_ctx, end_ctx,
                                    out, taps, call);
}

extern "C" int gss_enhance_observation_pcm16(gss_ctx *ctx, const gss_params *p,
                                             const int16_t *obs, int D, int64_t N,
                                             const uint8_t *act, int K, int64_t N_act, int target,
                                             int64_t start_ctx, int64_t end_ctx, double *out,
                                             const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    PipelineCall call;
    call.obs_type = 1;
    return enhance_observation_impl(ctx, p, obs, D, N, act, K, N_act, target, start_ctx, end_ctx,
                                    out, taps, call);
}

extern "C" int gss_enhance_observation_select(gss_ctx *ctx, const gss_params *p,
                                              const double *obs, int D, int64_t N,
                                              const uint8_t *act, int K, int64_t N_act,
                                              int target, int64_t start_ctx, int64_t end_ctx,
                                              const gss_channel_select *sel, double *out,
                                              const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    PipelineCall call;
    call.entry = "gss_enhance_observation_select";
    call.select = true;
    call.sel = sel;
    return enhance_observation_impl(ctx, p, obs, D, N, act, K, N_act, target, start_ctx, end_ctx,
                                    out, taps, call);
}

extern "C" int gss_enhance_observation_select_pcm16(gss_ctx *ctx, const gss_params *p,
                                                    const int16_t *obs, int D, int64_t N,
                                                    const uint8_t *act, int K, int64_t N_act,
                                                    int target, int64_t start_ctx,
                                                    int64_t end_ctx,
                                                    const gss_channel_select *sel, double *out,
                                                    const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    PipelineCall call;
    call.entry = "gss_enhance_observation_select";
    call.obs_type = 1;
    call.select = true;
    call.sel = sel;
    return enhance_observation_impl(ctx, p, obs, D, N, act, K, N_act, target, start_ctx, end_ctx,
                                    out, taps, call);
}

extern "C" int gss_enhance_observation_targets(gss_ctx *ctx, const gss_params *p,
                                               const double *obs, int D, int64_t N,
                                               const uint8_t *act, int K, int64_t N_act, int S,
                                               const int32_t *targets, const int64_t *start_ctx,
                                               const int64_t *end_ctx, double *out,
                                               const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    return enhance_observation_targets_impl(ctx, p, obs, 0, D, N, act, K, N_act, S, targets,
                                            start_ctx, end_ctx, out, taps);
}

extern "C" int gss_enhance_observation_targets_pcm16(gss_ctx *ctx, const gss_params *p,
                                                     const int16_t *obs, int D, int64_t N,
                                                     const uint8_t *act, int K, int64_t N_act,
                                                     int S, const int32_t *targets,
                                                     const int64_t *start_ctx,
                                                     const int64_t *end_ctx, double *out,
                                                     const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    return enhance_observation_targets_impl(ctx, p, obs, 1, D, N, act, K, N_act, S, targets,
                                            start_ctx, end_ctx, out, taps);
}

extern "C" int gss_separate_observation(gss_ctx *ctx, const gss_params *p, const double *obs,
                                        int D, int64_t N, const double *init, int K, double *out,
                                        double *prior, double *power, double *gamma,
                                        const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    const char *what = "gss_separate_observation";
    ctx->last_targets = 0;
    GSS_REQUIRE(ctx, p, GSS_ERR_INVALID, "%s: params is NULL", what);
    GSS_REQUIRE(ctx, prior, GSS_ERR_INVALID, "%s: prior_dev is NULL", what);
    GSS_TRY(check_pipeline_front(ctx, p, obs, D, N, init, out, what));
    GSS_REQUIRE(ctx, !(p->wpe && p->wpe_arrays > 1), GSS_ERR_UNSUPPORTED,
                "%s: wpe_arrays=%d, the per-array WPE has no annotation-free form", what,
                p->wpe_arrays);
    GSS_REQUIRE(ctx, !taps || !taps->act_frames, GSS_ERR_INVALID,
                "%s: taps->act_frames must be NULL (there is no frame activity)", what);
    GSS_TRY(check_class_count(ctx, K));
    int64_t T, T_act;
    GSS_TRY(check_pipeline_rest(ctx, p, D, N, K, N, &T, &T_act));
    const int F = p->stft_size / 2 + 1, S = K;

    PipelineCall call;
    call.entry = what;
    call.blind_init = init;
    call.blind_prior = prior;
    GSS_TRY(arena_reserve(ctx, targets_workspace(p, F, T, T_act, D, K, S, /*blind=*/true)));
    Workspace ws(ctx);
    const PipelineBuffers fr = pipeline_blocks(ws, p, F, T, T_act, D, K, S, call);
    GSS_TRY(ws.status(what));
    const size_t mark = ctx->arena_off;
    GSS_TRY(run_front(ctx, p, call, obs, D, D, N, nullptr, K, N, F, T, T_act, fr, mark, EmGuide{}));
    if (power) {     // (reads X and gamma; the scores are not asked for)
        double *scores = separate_scores_blocks(ws, K, T);
        GSS_TRY(ws.status(what));
        GSS_TRY(pact_run(ctx, fr.X, fr.gamma, F, K, T, D, nullptr, scores, power));
        GSS_TRY(arena_release(ctx, mark));
    }
    GSS_TRY(copy_tap(ctx, gamma, fr.gamma, sizeof(double) * (size_t)F * K * T));
    int32_t targets[GSS_MAX_CLASSES];
    for (int s = 0; s < S; ++s) targets[s] = s;
    return run_targets_tail(ctx, p, fr, F, T, T_act, D, K, S, targets, nullptr, nullptr, mark, out,
                            taps);
}

extern "C" int gss_enhance_observation_host(gss_ctx *ctx, const gss_params *p,
                                            const double *obs, int D, int64_t N,
                                            const uint8_t *act, int K, int64_t N_act,
                                            int target, int64_t start_ctx, int64_t end_ctx,
                                            double *out) {
    GSS_ENTER_VARIANTS(ctx);
    GSS_REQUIRE(ctx, p && obs && act && out && N >= 1 && D >= 1 && K >= 1, GSS_ERR_INVALID,
                "gss_enhance_observation_host: bad arguments");
    const int64_t T = gss_stft_num_frames(N, p->stft_size, p->stft_shift, p->stft_fading);
    const int64_t n_out = gss_istft_num_samples(T, p->stft_size, p->stft_shift, p->stft_fading);
    double *obs_d = nullptr, *out_d = nullptr;
    uint8_t *act_d = nullptr;
    int st = gss_dev_malloc(ctx, sizeof(double) * (size_t)D * N, (void **)&obs_d);
    if (st == GSS_OK) st = gss_dev_malloc(ctx, (size_t)K * N_act, (void **)&act_d);
    if (st == GSS_OK) st = gss_dev_malloc(ctx, sizeof(double) * (size_t)n_out, (void **)&out_d);
    if (st == GSS_OK) st = gss_memcpy_h2d(ctx, obs_d, obs, sizeof(double) * (size_t)D * N);
    if (st == GSS_OK) st = gss_memcpy_h2d(ctx, act_d, act, (size_t)K * N_act);
    if (st == GSS_OK)
        st = gss_enhance_observation(ctx, p, obs_d, D, N, act_d, K, N_act, target, start_ctx,
                                     end_ctx, out_d, nullptr);
    if (st == GSS_OK) st = gss_memcpy_d2h(ctx, out, out_d, sizeof(double) * (size_t)n_out);
    std::string keep = ctx->error;
    (void)hipStreamSynchronize(ctx->stream);
    if (obs_d) (void)hipFree(obs_d);
    if (act_d) (void)hipFree(act_d);
    if (out_d) (void)hipFree(out_d);
    ctx->error = keep;
    return st;
}

// ------------------------------------------------------------------ sample-block stream
// The stream state against the context's windows, before any launch.
static int check_stream_state(gss_ctx *ctx, const char *what, const gss_stream_state *s) {
    GSS_REQUIRE(ctx, s, GSS_ERR_INVALID, "%s: state is NULL", what);
    GSS_TRY(check_windows(ctx));
    GSS_REQUIRE(ctx, s->x_hist, GSS_ERR_INVALID, "%s: state->x_hist is NULL", what);
    GSS_REQUIRE(ctx, s->ola_tail, GSS_ERR_INVALID, "%s: state->ola_tail is NULL", what);
    GSS_REQUIRE(ctx, s->size == ctx->stft_size && s->shift == ctx->stft_shift, GSS_ERR_INVALID,
                "%s: state of stft %d/%d, gss_set_windows() has %d/%d", what, (int)s->size,
                (int)s->shift, ctx->stft_size, ctx->stft_shift);
    GSS_REQUIRE(ctx, s->shift < s->size, GSS_ERR_UNSUPPORTED,
                "%s: shift = size = %d, a stream needs overlapping frames", what, (int)s->size);
    GSS_REQUIRE(ctx, s->D >= 1 && s->D <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED,
                "%s: state->D = %d outside [1, %d]", what, (int)s->D, GSS_MAX_CHANNELS);
    GSS_REQUIRE(ctx, s->K >= 0 && s->K <= GSS_MAX_CLASSES, GSS_ERR_UNSUPPORTED,
                "%s: state->K = %d outside [0, %d]", what, (int)s->K, GSS_MAX_CLASSES);
    GSS_REQUIRE(ctx, (s->K > 0) == (s->act_hist != nullptr), GSS_ERR_INVALID,
                "%s: state->act_hist and state->K = %d disagree", what, (int)s->K);
    GSS_REQUIRE(ctx, s->received >= 0 && s->frames_out >= 0 &&
                         s->frames_out <= s->received / s->shift,
                GSS_ERR_INVALID, "%s: state counters received = %lld, frames_out = %lld", what,
                (long long)s->received, (long long)s->frames_out);
    return GSS_OK;
}

extern "C" int gss_stream_init(gss_ctx *ctx, gss_stream_state *state) {
    GSS_ENTER(ctx);
    GSS_TRY(check_stream_state(ctx, "gss_stream_init", state));
    return stream_init_run(ctx, state);
}

// The analysis arguments of a block, before any launch (act NULL: no activity in this call).
static int check_stream_input(gss_ctx *ctx, const char *what, const void *x, int in_type,
                              const uint8_t *act, int64_t n, const gss_stream_state *s) {
    GSS_TRY(check_stream_state(ctx, what, s));
    GSS_REQUIRE(ctx, x, GSS_ERR_INVALID, "%s: x_dev is NULL", what);
    GSS_REQUIRE(ctx, in_type == 0 || in_type == 1, GSS_ERR_INVALID, "%s: sample type %d", what,
                in_type);
    GSS_REQUIRE(ctx, n >= 0, GSS_ERR_INVALID, "%s: n = %lld is negative", what, (long long)n);
    GSS_REQUIRE(ctx, !act || s->act_hist, GSS_ERR_INVALID,
                "%s: act_dev given, the state carries no activity (state->K = 0)", what);
    GSS_REQUIRE(ctx, act || !s->act_hist, GSS_ERR_INVALID,
                "%s: act_dev is NULL, the state carries the activity of %d classes", what, (int)s->K);
    const int64_t Tn = gss_stream_num_frames(s->received, n, s->size, s->shift);
    GSS_REQUIRE(ctx, Tn < 2147483647, GSS_ERR_UNSUPPORTED, "%s: too many frames", what);
    GSS_TRY(check_stft_bins(ctx, s->size / 2 + 1, Tn, s->D));
    return GSS_OK;
}

extern "C" int gss_stft_stream(gss_ctx *ctx, const void *x, int in_type, const uint8_t *act,
                               int64_t n, gss_stream_state *state, gss_cplx *Y, uint8_t *actf) {
    GSS_ENTER(ctx);
    const char *const what = "gss_stft_stream";
    GSS_TRY(check_stream_input(ctx, what, x, in_type, act, n, state));
    GSS_REQUIRE(ctx, Y, GSS_ERR_INVALID, "%s: Y_dev is NULL", what);
    GSS_REQUIRE(ctx, !act || actf, GSS_ERR_INVALID, "%s: act_frames_dev is NULL", what);
    if (n == 0) return GSS_OK;
    const int64_t Tn = gss_stream_num_frames(state->received, n, state->size, state->shift);
    GSS_TRY(arena_reserve(ctx, stream_stft_workspace_bytes(Tn, state->D, state->K, state->size,
                                                           state->shift)));
    return stream_stft_run(ctx, x, in_type, act, n, state, reinterpret_cast<cplx *>(Y), actf);
}

// The synthesis arguments, before any launch: gss_istft_stream's rules, and with `targets` those
// of gss_istft_stream_targets' S signals and their tails, each in its place.
static int check_istft_stream(gss_ctx *ctx, const char *what, const gss_stream_state *state,
                              const gss_cplx *X, int64_t Tn, const double *out, bool targets,
                              int S, const double *tails) {
    GSS_TRY(check_stream_state(ctx, what, state));
    GSS_REQUIRE(ctx, X, GSS_ERR_INVALID, "%s: X_dev is NULL", what);
    if (targets) GSS_REQUIRE(ctx, tails, GSS_ERR_INVALID, "%s: tails_dev is NULL", what);
    GSS_REQUIRE(ctx, out, GSS_ERR_INVALID, "%s: out_dev is NULL", what);
    if (targets) {
        GSS_REQUIRE(ctx, S >= 1 && S <= GSS_CACGMM_ONLINE_MAX_CLASSES, GSS_ERR_INVALID,
                    "%s: S = %d outside [1, %d]", what, S, GSS_CACGMM_ONLINE_MAX_CLASSES);
        GSS_REQUIRE(ctx, tails != state->ola_tail, GSS_ERR_INVALID,
                    "%s: tails_dev is the stream state's own ola_tail", what);
    }
    GSS_REQUIRE(ctx, Tn >= 0, GSS_ERR_INVALID, "%s: Tn = %lld is negative", what, (long long)Tn);
    GSS_REQUIRE(ctx, state->frames_out + Tn <= state->received / state->shift, GSS_ERR_INVALID,
                "%s: Tn = %lld frames after %lld, the stream has analysed %lld", what, (long long)Tn,
                (long long)state->frames_out, (long long)(state->received / state->shift));
    if (targets)
        GSS_REQUIRE(ctx, (int64_t)S * Tn < 2147483647, GSS_ERR_UNSUPPORTED, "%s: too many frames",
                    what);
    return GSS_OK;
}

extern "C" int gss_istft_stream(gss_ctx *ctx, const gss_cplx *X, int64_t Tn, gss_stream_state *state,
                                double *out) {
    GSS_ENTER(ctx);
    GSS_TRY(check_istft_stream(ctx, "gss_istft_stream", state, X, Tn, out, false, 1, nullptr));
    if (Tn == 0) return GSS_OK;
    GSS_TRY(arena_reserve(ctx, stream_istft_targets_workspace_bytes(Tn, 1, state->size, state->shift)));
    return stream_istft_targets_run(ctx, reinterpret_cast<const cplx *>(X), Tn, 1, state,
                                    state->ola_tail, out);
}

extern "C" int gss_istft_stream_targets(gss_ctx *ctx, const gss_cplx *X, int64_t Tn, int S,
                                        gss_stream_state *state, double *tails, double *out) {
    GSS_ENTER(ctx);
    GSS_TRY(check_istft_stream(ctx, "gss_istft_stream_targets", state, X, Tn, out, true, S, tails));
    if (Tn == 0) return GSS_OK;
    GSS_TRY(arena_reserve(ctx, stream_istft_targets_workspace_bytes(Tn, S, state->size, state->shift)));
    return stream_istft_targets_run(ctx, reinterpret_cast<const cplx *>(X), Tn, S, state, tails, out);
}

// The argument rules gss_stream_block and gss_stream_block_targets share, before any launch, in
// two halves around the rules of the beamformer states and the targets.
static int check_stream_block_head(gss_ctx *ctx, const char *what, const gss_params *p,
                                   const gss_stream_cfg *cfg, const gss_stream_state *st,
                                   const gss_cacgmm_online_state *em, const void *bf, const void *x,
                                   int in_type, const uint8_t *act, int64_t n, const double *out) {
    GSS_REQUIRE(ctx, cfg, GSS_ERR_INVALID, "%s: cfg is NULL", what);
    GSS_REQUIRE(ctx, em, GSS_ERR_INVALID, "%s: the CACGMM state is NULL", what);
    GSS_REQUIRE(ctx, bf, GSS_ERR_INVALID, "%s: the MVDR state is NULL", what);
    GSS_REQUIRE(ctx, out, GSS_ERR_INVALID, "%s: out_dev is NULL", what);
    GSS_TRY(check_windows(ctx));
    GSS_TRY(check_params(ctx, p));
    GSS_REQUIRE(ctx, p->stft_fading == 1, GSS_ERR_UNSUPPORTED,
                "%s: stft_fading = %d, a stream is the faded STFT", what, p->stft_fading);
    GSS_REQUIRE(ctx, p->bf == 0, GSS_ERR_UNSUPPORTED,
                "%s: bf=%d, only 0 ('mvdrSouden_ban') has an online form", what, p->bf);
    GSS_TRY(check_stream_input(ctx, what, x, in_type, act, n, st));
    const int D = st->D, K = em->K, F = p->stft_size / 2 + 1;
    GSS_TRY(check_em_online_shape(ctx, what, F, K, D));
    GSS_TRY(check_cacgmm_online_state(ctx, what, em, F, K, D));
    GSS_REQUIRE(ctx, !act || st->K == K, GSS_ERR_INVALID,
                "%s: the stream carries the activity of %d classes, the CACGMM state has %d", what,
                (int)st->K, K);
    return GSS_OK;
}

static int check_stream_block_tail(gss_ctx *ctx, const char *what, const gss_params *p,
                                   const gss_stream_cfg *cfg, const gss_stream_state *st,
                                   const gss_wpe_online_state *wpe) {
    const int D = st->D, F = p->stft_size / 2 + 1;
    const gss_em_online em_cfg{cfg->em_forget, 1.0};
    GSS_TRY(check_em_online(ctx, what, &em_cfg));
    const gss_bf_online bf_cfg{cfg->bf_forget, 1.0, cfg->ref_channel, 0, 1.0};
    GSS_REQUIRE(ctx, cfg->ref_channel >= 0, GSS_ERR_INVALID,
                "%s: ref_channel = %d, a stream has no window to choose one over", what,
                (int)cfg->ref_channel);
    GSS_TRY(check_bf_online(ctx, what, &bf_cfg, D));
    GSS_REQUIRE(ctx, (wpe != nullptr) == (p->wpe != 0), GSS_ERR_INVALID,
                "%s: params->wpe = %d %s a WPE state", what, p->wpe, wpe ? "with" : "without");
    if (p->wpe) {
        const int A = wpe_arrays_of(p);
        GSS_TRY(check_wpe_online_state(ctx, what, wpe));
        GSS_TRY(check_wpe_arrays(ctx, p, D));
        GSS_TRY(check_wpe_online(ctx, what, F, A, D / A, p->wpe_taps, p->wpe_delay, cfg->wpe_alpha));
    }
    return GSS_OK;
}

// ------------------------------------------------------------------ S targets of one stream
// The targets and their beamformer states, before any launch: 1 <= S <= 8 distinct classes of
// [0, K), S states of the call's F and D, no buffer handed in twice.
static int check_online_targets(gss_ctx *ctx, const char *what, const int32_t *targets, int S, int K,
                                const gss_mvdr_online_state *states, int F, int D) {
    GSS_REQUIRE(ctx, S >= 1 && S <= GSS_CACGMM_ONLINE_MAX_CLASSES, GSS_ERR_INVALID,
                "%s: S = %d outside [1, %d]", what, S, GSS_CACGMM_ONLINE_MAX_CLASSES);
    GSS_REQUIRE(ctx, targets, GSS_ERR_INVALID, "%s: targets is NULL", what);
    GSS_REQUIRE(ctx, states, GSS_ERR_INVALID, "%s: the MVDR states are NULL", what);
    for (int s = 0; s < S; ++s) {
        GSS_TRY(check_target_index(ctx, targets[s], K));
        for (int r = 0; r < s; ++r)
            GSS_REQUIRE(ctx, targets[r] != targets[s], GSS_ERR_INVALID,
                        "%s: target %d is given twice (targets[%d] and targets[%d])", what,
                        (int)targets[s], r, s);
        GSS_TRY(check_mvdr_online_state(ctx, what, &states[s], F, D));
        for (int r = 0; r < s; ++r)
            GSS_REQUIRE(ctx, states[r].phi_x != states[s].phi_x && states[r].phi_x != states[s].phi_n &&
                                 states[r].phi_n != states[s].phi_x && states[r].phi_n != states[s].phi_n,
                        GSS_ERR_INVALID, "%s: states[%d] and states[%d] share a buffer", what, r, s);
    }
    return GSS_OK;
}

struct OnlineTargetStates {
    cplx *phi_x[GSS_CACGMM_ONLINE_MAX_CLASSES], *phi_n[GSS_CACGMM_ONLINE_MAX_CLASSES];
    OnlineTargetStates(const gss_mvdr_online_state *states, int S) {
        for (int s = 0; s < S; ++s) {
            phi_x[s] = reinterpret_cast<cplx *>(states[s].phi_x);
            phi_n[s] = reinterpret_cast<cplx *>(states[s].phi_n);
        }
    }
};

extern "C" int gss_mvdr_online_targets(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                                       const double *gamma, int K, const int32_t *targets, int S,
                                       int ban, const gss_bf_online *cfg,
                                       const gss_mvdr_online_state *states, int postfilter,
                                       double *mx, double *mn, gss_cplx *Xhat, gss_cplx *W) {
    GSS_ENTER(ctx);
    const char *const what = "gss_mvdr_online_targets";
    GSS_REQUIRE(ctx, Y, GSS_ERR_INVALID, "%s: Y_dev is NULL", what);
    GSS_REQUIRE(ctx, gamma, GSS_ERR_INVALID, "%s: gamma_dev is NULL", what);
    GSS_REQUIRE(ctx, Xhat, GSS_ERR_INVALID, "%s: Xhat_dev is NULL", what);
    GSS_REQUIRE(ctx, T >= 0, GSS_ERR_INVALID, "%s: T = %lld is negative", what, (long long)T);
    GSS_REQUIRE(ctx, postfilter == 0 || postfilter == 1, GSS_ERR_INVALID, "%s: postfilter = %d", what,
                postfilter);
    GSS_TRY(check_em_online_shape(ctx, what, F, K, D));
    GSS_TRY(check_bf_online(ctx, what, cfg, D));
    GSS_REQUIRE(ctx, cfg->ref_channel >= 0, GSS_ERR_INVALID,
                "%s: ref_channel = %d, the targets of a stream have no window to choose one over",
                what, (int)cfg->ref_channel);
    GSS_TRY(check_online_targets(ctx, what, targets, S, K, states, F, D));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    GSS_REQUIRE(ctx, !W || (int64_t)S * F * T * D < (1LL << 31), GSS_ERR_UNSUPPORTED,
                "%s: S * F * T * D is 2^31 or more", what);
    if (T == 0) return GSS_OK;
    GSS_TRY(arena_reserve(ctx, mvdr_online_targets_workspace_bytes(F, S)));
    ctx->last_online_targets = S;
    const OnlineTargetStates st(states, S);
    return mvdr_online_targets_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, gamma, K, targets,
                                   S, ban != 0, cfg->forget, cfg->ref_channel, st.phi_x, st.phi_n,
                                   postfilter, mx, mn, reinterpret_cast<cplx *>(Xhat),
                                   reinterpret_cast<cplx *>(W), nullptr);
}

extern "C" int gss_last_mvdr_online_fallbacks_targets(gss_ctx *ctx, int64_t *counts, int S) {
    GSS_ENTER(ctx);
    const char *const what = "gss_last_mvdr_online_fallbacks_targets";
    GSS_REQUIRE(ctx, counts, GSS_ERR_INVALID, "%s: NULL", what);
    GSS_REQUIRE(ctx, S >= 1 && S <= ctx->last_online_targets, GSS_ERR_INVALID,
                "%s: S = %d, the last online MVDR targets call had %d target(s)", what, S,
                ctx->last_online_targets);
    GSS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < S; ++s)
        counts[s] = __atomic_load_n(ctx->status_host + GSS_STATUS_MVDR_ONLINE_TARGETS + s,
                                    __ATOMIC_ACQUIRE);
    return GSS_OK;
}

// The buffers of one block of a stream of S targets, taken first; every stage runs above them.
// The mask table exists for the taps and for the one-target entry, whose beamformer reads it.
struct StreamBlockBuffers {
    cplx *Y, *X;        // the block's STFT and the WPE output; no WPE: X is Y
    uint8_t *actf;      // (K,Tn), NULL for an unguided stream
    double *gamma;
    double *mx, *mn;    // (S,F,Tn) each, or NULL
    cplx *Xhat;         // (S,Tn,F)
    int32_t *ref;       // (S,)
};
static StreamBlockBuffers stream_block_blocks(Workspace &ws, bool wpe, bool guided, bool masks,
                                              int F, int64_t Tn, int D, int K, int S) {
    const size_t ft = (size_t)F * Tn;
    StreamBlockBuffers b;
    b.Y = ws.take<cplx>(ft * D, "stream Y");
    b.X = wpe ? ws.take<cplx>(ft * D, "stream X") : b.Y;
    b.actf = guided ? ws.take<uint8_t>((size_t)K * Tn, "stream frame activity") : nullptr;
    b.gamma = ws.take<double>(ft * K, "stream gamma");
    b.mx = masks ? ws.take<double>(ft * S, "stream target masks") : nullptr;
    b.mn = masks ? ws.take<double>(ft * S, "stream distortion masks") : nullptr;
    b.Xhat = ws.take<cplx>(ft * S, "stream Xhat of the targets");
    b.ref = ws.take<int32_t>(GSS_CACGMM_ONLINE_MAX_CLASSES, "stream refs");
    return b;
}

static size_t stream_block_workspace(const gss_params *p, bool guided, bool masks, int F, int64_t Tn,
                                     int D, int K, int S) {
    size_t stage = stream_stft_workspace_bytes(Tn, D, guided ? K : 0, p->stft_size, p->stft_shift);
    if (Tn == 0) return stage + (1 << 16);
    Workspace ws;
    stream_block_blocks(ws, p->wpe != 0, guided, masks, F, Tn, D, K, S);
    if (p->wpe)
        stage = std::max(stage, wpe_online_workspace_bytes(F, Tn, wpe_arrays_of(p), D / wpe_arrays_of(p),
                                                           p->wpe_taps, p->wpe_delay, false));
    stage = std::max(stage, cacgmm_online_workspace_bytes(F, K, D, false));
    stage = std::max(stage, mvdr_online_workspace_bytes(F, Tn, D, false, false));
    stage = std::max(stage, mvdr_online_targets_workspace_bytes(F, S));
    stage = std::max(stage, stream_istft_targets_workspace_bytes(Tn, S, p->stft_size, p->stft_shift));
    return ws.bytes + 4096 + stage + (1 << 16);
}

// The stages of a block that do not depend on the targets, above the block's buffers: the
// analysis, the online WPE and the online CACGMM -> b.X and the posteriors b.gamma.
static int stream_block_front(gss_ctx *ctx, const gss_params *p, const gss_stream_cfg *cfg,
                              gss_stream_state *st, const gss_wpe_online_state *wpe,
                              gss_cacgmm_online_state *em, const void *x, int in_type,
                              const uint8_t *act, int64_t n, int64_t Tn, const StreamBlockBuffers &b,
                              size_t mark) {
    const int D = st->D, K = em->K, F = p->stft_size / 2 + 1;
    const int A = wpe_arrays_of(p);
    GSS_TRY(stream_stft_run(ctx, x, in_type, act, n, st, b.Y, b.actf));
    GSS_TRY(arena_release(ctx, mark));
    // no solve in this call: clear the pivot count an earlier utterance left behind
    GSS_HIP_CHECK(ctx, hipMemsetAsync(ctx->status_dev + GSS_STATUS_WPE_ZERO_PIVOTS, 0,
                                      sizeof(int32_t), ctx->stream));
    if (p->wpe) {
        GSS_TRY(wpe_online_run(ctx, b.Y, F, Tn, A, D / A, p->wpe_taps, p->wpe_delay, cfg->wpe_alpha,
                               reinterpret_cast<cplx *>(wpe->inv_cov_dev),
                               reinterpret_cast<cplx *>(wpe->filter_dev),
                               reinterpret_cast<cplx *>(wpe->history_dev), b.X,
                               gss_variant_set("wpe_online_mem")));
        GSS_TRY(arena_release(ctx, mark));
    }
    const EmGuide guide = act ? em_guide_from_activity(b.actf, Tn) : EmGuide{};
    GSS_TRY(cacgmm_online_run(ctx, b.X, F, Tn, D, guide, K, cfg->em_forget, 1.0,
                              reinterpret_cast<cplx *>(em->s), em->n, b.gamma));
    return arena_release(ctx, mark);
}

// One block of a stream for S targets (the arguments validated by the entry): the analysis, the
// online WPE and the online CACGMM once, then the beamformer and one synthesis for the S targets.
// gss_stream_block is S = 1 with tails = the stream state's own ola_tail and `one_target`: its
// beamformer stage is the mask launch, mvdr_online_kernel and the postfilter launch, not the
// targets kernel with S = 1, which was measured 0.4 ms slower over the 625 frames of a
// 160 000-sample block at D = 4; the bits are the same.
static int stream_block_impl(gss_ctx *ctx, const char *what, const gss_params *p,
                             const gss_stream_cfg *cfg, gss_stream_state *st,
                             const gss_wpe_online_state *wpe, gss_cacgmm_online_state *em,
                             const void *x, int in_type, const uint8_t *act, int64_t n,
                             const int32_t *targets, int S, const gss_mvdr_online_state *states,
                             double *tails, double *out, const gss_debug_taps *taps,
                             bool one_target) {
    const int D = st->D, K = em->K, F = p->stft_size / 2 + 1;
    const bool guided = act != nullptr;
    if (n == 0) return GSS_OK;

    const int64_t Tn = gss_stream_num_frames(st->received, n, p->stft_size, p->stft_shift);
    GSS_REQUIRE(ctx, (int64_t)S * Tn < 2147483647, GSS_ERR_UNSUPPORTED, "%s: too many frames", what);
    const bool masks = one_target || (taps && (taps->target_mask || taps->distortion_mask));
    GSS_TRY(arena_reserve(ctx, stream_block_workspace(p, guided, masks, F, Tn, D, K, S)));
    if (Tn == 0)    // the samples enter the history, no frame is complete yet
        return stream_stft_run(ctx, x, in_type, act, n, st, nullptr, nullptr);
    Workspace ws(ctx);
    const StreamBlockBuffers b = stream_block_blocks(ws, p->wpe != 0, guided, masks, F, Tn, D, K, S);
    GSS_TRY(ws.status(what));
    const size_t mark = ctx->arena_off;
    GSS_TRY(stream_block_front(ctx, p, cfg, st, wpe, em, x, in_type, act, n, Tn, b, mark));
    const OnlineTargetStates bf(states, S);
    if (one_target) {
        GSS_TRY(masks_from_posteriors_run(ctx, b.gamma, F, K, Tn, targets[0], /*drop=*/0, 0, 0, b.mx,
                                          b.mn));
        GSS_TRY(mvdr_online_run(ctx, b.X, F, Tn, D, b.mx, b.mn, /*ban=*/1, cfg->bf_forget, 1.0,
                                cfg->ref_channel, bf.phi_x[0], bf.phi_n[0], b.Xhat, 1, F, nullptr,
                                b.ref));
        GSS_TRY(arena_release(ctx, mark));
        if (p->postfilter == 1) GSS_TRY(mask_mul_run(ctx, b.Xhat, b.mx, F, Tn));
    } else {
        GSS_TRY(mvdr_online_targets_run(ctx, b.X, F, Tn, D, b.gamma, K, targets, S, /*ban=*/1,
                                        cfg->bf_forget, cfg->ref_channel, bf.phi_x, bf.phi_n,
                                        p->postfilter == 1, b.mx, b.mn, b.Xhat, nullptr, b.ref));
        GSS_TRY(arena_release(ctx, mark));
    }
    GSS_TRY(stream_istft_targets_run(ctx, b.Xhat, Tn, S, st, tails, out));
    if (taps) {
        const size_t ft = (size_t)F * Tn;
        GSS_TRY(copy_tap(ctx, taps->Obs_ftd, b.X, sizeof(cplx) * ft * D));
        if (guided) GSS_TRY(copy_tap(ctx, taps->act_frames, b.actf, (size_t)K * Tn));
        GSS_TRY(copy_tap(ctx, taps->gamma, b.gamma, sizeof(double) * ft * K));
        GSS_TRY(copy_tap(ctx, taps->target_mask, b.mx, sizeof(double) * ft * S));
        GSS_TRY(copy_tap(ctx, taps->distortion_mask, b.mn, sizeof(double) * ft * S));
        GSS_TRY(copy_tap(ctx, taps->Xhat, b.Xhat, sizeof(cplx) * ft * S));
        GSS_TRY(copy_tap(ctx, taps->ref_channel, b.ref, sizeof(int32_t) * S));
    }
    return GSS_OK;
}

extern "C" int gss_stream_block(gss_ctx *ctx, const gss_params *p, const gss_stream_cfg *cfg,
                                gss_stream_state *st, const gss_wpe_online_state *wpe,
                                gss_cacgmm_online_state *em, gss_mvdr_online_state *bf, const void *x,
                                int in_type, const uint8_t *act, int64_t n, int target, double *out,
                                const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    const char *const what = "gss_stream_block";
    GSS_TRY(check_stream_block_head(ctx, what, p, cfg, st, em, bf, x, in_type, act, n, out));
    GSS_TRY(check_mvdr_online_state(ctx, what, bf, p->stft_size / 2 + 1, st->D));
    GSS_TRY(check_target_index(ctx, target, em->K));
    GSS_TRY(check_stream_block_tail(ctx, what, p, cfg, st, wpe));
    const int32_t targets[1] = {target};
    return stream_block_impl(ctx, what, p, cfg, st, wpe, em, x, in_type, act, n, targets, 1, bf,
                             st->ola_tail, out, taps, /*one_target=*/true);
}

extern "C" int gss_stream_block_targets(gss_ctx *ctx, const gss_params *p, const gss_stream_cfg *cfg,
                                        gss_stream_state *st, const gss_wpe_online_state *wpe,
                                        gss_cacgmm_online_state *em,
                                        const gss_mvdr_online_state *bf, double *tails, const void *x,
                                        int in_type, const uint8_t *act, int64_t n,
                                        const int32_t *targets, int S, double *out,
                                        const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    const char *const what = "gss_stream_block_targets";
    GSS_TRY(check_stream_block_head(ctx, what, p, cfg, st, em, bf, x, in_type, act, n, out));
    GSS_REQUIRE(ctx, tails, GSS_ERR_INVALID, "%s: tails_dev is NULL", what);
    GSS_REQUIRE(ctx, tails != st->ola_tail, GSS_ERR_INVALID,
                "%s: tails_dev is the stream state's own ola_tail", what);
    GSS_TRY(check_online_targets(ctx, what, targets, S, em->K, bf, p->stft_size / 2 + 1, st->D));
    GSS_TRY(check_stream_block_tail(ctx, what, p, cfg, st, wpe));
    // a block that completes a frame runs the beamformer: S targets for the per-target counts
    if (gss_stream_num_frames(st->received, n, p->stft_size, p->stft_shift) > 0)
        ctx->last_online_targets = S;
    return stream_block_impl(ctx, what, p, cfg, st, wpe, em, x, in_type, act, n, targets, S, bf, tails,
                             out, taps, /*one_target=*/false);
}

// ------------------------------------------------------------------ online MVDR with a look-ahead
// A delay line (or S of them), before any launch: the buffers, the sizes of the call, L within the
// bound, the host counter within [0, L]; S lines share L and `held` and no buffer.
static int check_mvdr_online_holds(gss_ctx *ctx, const char *what, const gss_mvdr_online_hold *holds,
                                   int S, int F, int D) {
    GSS_REQUIRE(ctx, holds, GSS_ERR_INVALID, "%s: hold is NULL", what);
    for (int s = 0; s < S; ++s) {
        const gss_mvdr_online_hold &h = holds[s];
        GSS_REQUIRE(ctx, h.frames, GSS_ERR_INVALID, "%s: hold->frames is NULL", what);
        GSS_REQUIRE(ctx, h.mask, GSS_ERR_INVALID, "%s: hold->mask is NULL", what);
        GSS_REQUIRE(ctx, h.filter, GSS_ERR_INVALID, "%s: hold->filter is NULL", what);
        GSS_REQUIRE(ctx, h.frames != h.filter, GSS_ERR_INVALID,
                    "%s: hold->frames and hold->filter alias", what);
        GSS_REQUIRE(ctx, h.F == F && h.D == D, GSS_ERR_INVALID,
                    "%s: hold of F = %d, D = %d in a call of F = %d, D = %d", what, (int)h.F, (int)h.D,
                    F, D);
        GSS_REQUIRE(ctx, h.L >= 1 && h.L <= GSS_MVDR_ONLINE_MAX_LOOKAHEAD, GSS_ERR_INVALID,
                    "%s: hold->L = %d outside [1, %d]", what, (int)h.L, GSS_MVDR_ONLINE_MAX_LOOKAHEAD);
        GSS_REQUIRE(ctx, h.held >= 0 && h.held <= h.L, GSS_ERR_INVALID,
                    "%s: hold->held = %d outside [0, %d]", what, (int)h.held, (int)h.L);
        GSS_REQUIRE(ctx, h.L == holds[0].L && h.held == holds[0].held, GSS_ERR_INVALID,
                    "%s: holds[%d] has L = %d, held = %d, holds[0] L = %d, held = %d", what, s,
                    (int)h.L, (int)h.held, (int)holds[0].L, (int)holds[0].held);
        for (int r = 0; r < s; ++r)
            GSS_REQUIRE(ctx, holds[r].frames != h.frames && holds[r].mask != h.mask &&
                                 holds[r].filter != h.filter && holds[r].frames != h.filter &&
                                 holds[r].filter != h.frames,
                        GSS_ERR_INVALID, "%s: holds[%d] and holds[%d] share a buffer", what, r, s);
    }
    return GSS_OK;
}

static int check_lookahead_ref(gss_ctx *ctx, const char *what, const gss_bf_online *cfg) {
    GSS_REQUIRE(ctx, cfg->ref_channel >= 0, GSS_ERR_INVALID,
                "%s: ref_channel = %d, the whole-window choice is per call and a delay line outlives "
                "a call", what, (int)cfg->ref_channel);
    return GSS_OK;
}

extern "C" int gss_mvdr_online_hold_init(gss_ctx *ctx, gss_mvdr_online_hold *hold) {
    GSS_ENTER(ctx);
    const char *const what = "gss_mvdr_online_hold_init";
    GSS_REQUIRE(ctx, hold, GSS_ERR_INVALID, "%s: hold is NULL", what);
    GSS_REQUIRE(ctx, hold->F >= 1, GSS_ERR_INVALID, "%s: F = %d is smaller than 1", what, (int)hold->F);
    GSS_REQUIRE(ctx, hold->D >= 1 && hold->D <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED,
                "%s: D = %d outside [1, %d]", what, (int)hold->D, GSS_MAX_CHANNELS);
    gss_mvdr_online_hold probe = *hold;
    probe.held = 0;
    GSS_TRY(check_mvdr_online_holds(ctx, what, &probe, 1, hold->F, hold->D));
    return mvdr_online_hold_init_run(ctx, hold);
}

extern "C" int gss_mvdr_online_lookahead(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T, int D,
                                         const double *mx, const double *mn, int ban,
                                         const gss_bf_online *cfg, gss_mvdr_online_state *state,
                                         gss_mvdr_online_hold *hold, gss_cplx *Xhat, gss_cplx *W,
                                         int64_t *frames_out) {
    GSS_ENTER(ctx);
    const char *const what = "gss_mvdr_online_lookahead";
    GSS_REQUIRE(ctx, Y, GSS_ERR_INVALID, "%s: Y_dev is NULL", what);
    GSS_REQUIRE(ctx, mx, GSS_ERR_INVALID, "%s: mask_x_dev is NULL", what);
    GSS_REQUIRE(ctx, mn, GSS_ERR_INVALID, "%s: mask_n_dev is NULL", what);
    GSS_REQUIRE(ctx, F >= 1, GSS_ERR_INVALID, "%s: F = %d is smaller than 1", what, F);
    GSS_REQUIRE(ctx, T >= 0, GSS_ERR_INVALID, "%s: T = %lld is negative", what, (long long)T);
    GSS_TRY(check_bf_online(ctx, what, cfg, D));
    GSS_TRY(check_lookahead_ref(ctx, what, cfg));
    GSS_REQUIRE(ctx, state, GSS_ERR_INVALID, "%s: state is NULL, a delay line needs the caller's",
                what);
    GSS_TRY(check_mvdr_online_state(ctx, what, state, F, D));
    GSS_TRY(check_mvdr_online_holds(ctx, what, hold, 1, F, D));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    const int64_t R = mvdr_online_lookahead_rows(hold, T);
    GSS_REQUIRE(ctx, Xhat || R == 0, GSS_ERR_INVALID, "%s: Xhat_dev is NULL", what);
    if (frames_out) *frames_out = R;
    if (T == 0) return GSS_OK;
    GSS_TRY(arena_reserve(ctx, mvdr_online_lookahead_workspace_bytes(F, 1)));
    return mvdr_online_lookahead_run(ctx, reinterpret_cast<const cplx *>(Y), F, T, D, mx, mn,
                                     ban != 0, cfg->forget, cfg->ref_channel,
                                     reinterpret_cast<cplx *>(state->phi_x),
                                     reinterpret_cast<cplx *>(state->phi_n), hold,
                                     reinterpret_cast<cplx *>(Xhat), reinterpret_cast<cplx *>(W));
}

extern "C" int gss_mvdr_online_lookahead_targets(gss_ctx *ctx, const gss_cplx *Y, int F, int64_t T,
                                                 int D, const double *gamma, int K,
                                                 const int32_t *targets, int S, int ban,
                                                 const gss_bf_online *cfg,
                                                 const gss_mvdr_online_state *states,
                                                 gss_mvdr_online_hold *holds, int postfilter,
                                                 double *mx, double *mn, gss_cplx *Xhat, gss_cplx *W,
                                                 int64_t *frames_out) {
    GSS_ENTER(ctx);
    const char *const what = "gss_mvdr_online_lookahead_targets";
    GSS_REQUIRE(ctx, Y, GSS_ERR_INVALID, "%s: Y_dev is NULL", what);
    GSS_REQUIRE(ctx, gamma, GSS_ERR_INVALID, "%s: gamma_dev is NULL", what);
    GSS_REQUIRE(ctx, T >= 0, GSS_ERR_INVALID, "%s: T = %lld is negative", what, (long long)T);
    GSS_REQUIRE(ctx, postfilter == 0 || postfilter == 1, GSS_ERR_INVALID, "%s: postfilter = %d", what,
                postfilter);
    GSS_TRY(check_em_online_shape(ctx, what, F, K, D));
    GSS_TRY(check_bf_online(ctx, what, cfg, D));
    GSS_TRY(check_lookahead_ref(ctx, what, cfg));
    GSS_TRY(check_online_targets(ctx, what, targets, S, K, states, F, D));
    GSS_TRY(check_mvdr_online_holds(ctx, what, holds, S, F, D));
    GSS_TRY(check_stft_bins(ctx, F, T, D));
    const int64_t R = mvdr_online_lookahead_rows(holds, T);
    GSS_REQUIRE(ctx, Xhat || R == 0, GSS_ERR_INVALID, "%s: Xhat_dev is NULL", what);
    GSS_REQUIRE(ctx, !W || (int64_t)S * F * R * D < (1LL << 31), GSS_ERR_UNSUPPORTED,
                "%s: S * F * R * D is 2^31 or more", what);
    if (frames_out) *frames_out = R;
    if (T == 0) return GSS_OK;
    GSS_TRY(arena_reserve(ctx, mvdr_online_lookahead_workspace_bytes(F, S)));
    ctx->last_online_targets = S;
    const OnlineTargetStates st(states, S);
    return mvdr_online_lookahead_targets_run(
        ctx, reinterpret_cast<const cplx *>(Y), F, T, D, gamma, K, targets, S, ban != 0, cfg->forget,
        cfg->ref_channel, st.phi_x, st.phi_n, holds, postfilter, mx, mn,
        reinterpret_cast<cplx *>(Xhat), R, reinterpret_cast<cplx *>(W), nullptr);
}

extern "C" int gss_mvdr_online_release(gss_ctx *ctx, gss_mvdr_online_hold *holds, int S,
                                       int postfilter, gss_cplx *Xhat, gss_cplx *W,
                                       int64_t *frames_out) {
    GSS_ENTER(ctx);
    const char *const what = "gss_mvdr_online_release";
    GSS_REQUIRE(ctx, S >= 1 && S <= GSS_CACGMM_ONLINE_MAX_CLASSES, GSS_ERR_INVALID,
                "%s: S = %d outside [1, %d]", what, S, GSS_CACGMM_ONLINE_MAX_CLASSES);
    GSS_REQUIRE(ctx, postfilter == 0 || postfilter == 1, GSS_ERR_INVALID, "%s: postfilter = %d", what,
                postfilter);
    GSS_REQUIRE(ctx, holds, GSS_ERR_INVALID, "%s: hold is NULL", what);
    GSS_REQUIRE(ctx, holds[0].F >= 1, GSS_ERR_INVALID, "%s: F = %d is smaller than 1", what,
                (int)holds[0].F);
    GSS_REQUIRE(ctx, holds[0].D >= 1 && holds[0].D <= GSS_MAX_CHANNELS, GSS_ERR_UNSUPPORTED,
                "%s: D = %d outside [1, %d]", what, (int)holds[0].D, GSS_MAX_CHANNELS);
    GSS_TRY(check_mvdr_online_holds(ctx, what, holds, S, holds[0].F, holds[0].D));
    const int64_t h = holds[0].held;
    GSS_REQUIRE(ctx, Xhat || h == 0, GSS_ERR_INVALID, "%s: Xhat_dev is NULL", what);
    if (frames_out) *frames_out = h;
    return mvdr_online_release_run(ctx, holds, S, postfilter, reinterpret_cast<cplx *>(Xhat), h,
                                   reinterpret_cast<cplx *>(W));
}

// The buffers of a look-ahead block: those of stream_block_blocks for the block's Tn frames, but
// Xhat holds the rows the block RELEASES (at most Tn + L per target).
static StreamBlockBuffers stream_lookahead_blocks(Workspace &ws, bool wpe, bool guided, bool masks,
                                                  int F, int64_t Tn, int64_t rows, int D, int K,
                                                  int S) {
    const size_t ft = (size_t)F * Tn;
    StreamBlockBuffers b{};
    if (Tn > 0) {
        b.Y = ws.take<cplx>(ft * D, "stream Y");
        b.X = wpe ? ws.take<cplx>(ft * D, "stream X") : b.Y;
        b.actf = guided ? ws.take<uint8_t>((size_t)K * Tn, "stream frame activity") : nullptr;
        b.gamma = ws.take<double>(ft * K, "stream gamma");
        b.mx = masks ? ws.take<double>(ft * S, "stream target masks") : nullptr;
        b.mn = masks ? ws.take<double>(ft * S, "stream distortion masks") : nullptr;
    }
    b.Xhat = rows > 0 ? ws.take<cplx>((size_t)F * rows * S, "stream Xhat released") : nullptr;
    b.ref = ws.take<int32_t>(GSS_CACGMM_ONLINE_MAX_CLASSES, "stream refs");
    return b;
}

extern "C" int gss_stream_block_lookahead(gss_ctx *ctx, const gss_params *p, const gss_stream_cfg *cfg,
                                          gss_stream_state *st, const gss_wpe_online_state *wpe,
                                          gss_cacgmm_online_state *em,
                                          const gss_mvdr_online_state *states,
                                          gss_mvdr_online_hold *holds, double *tails, const void *x,
                                          int in_type, const uint8_t *act, int64_t n,
                                          const int32_t *targets, int S, int release, double *out,
                                          int64_t *samples_out, const gss_debug_taps *taps) {
    GSS_ENTER_VARIANTS(ctx);
    const char *const what = "gss_stream_block_lookahead";
    GSS_TRY(check_stream_block_head(ctx, what, p, cfg, st, em, states, x, in_type, act, n, out));
    GSS_REQUIRE(ctx, tails, GSS_ERR_INVALID, "%s: tails_dev is NULL", what);
    GSS_REQUIRE(ctx, tails != st->ola_tail, GSS_ERR_INVALID,
                "%s: tails_dev is the stream state's own ola_tail", what);
    GSS_REQUIRE(ctx, release == 0 || release == 1, GSS_ERR_INVALID, "%s: release = %d", what, release);
    const int D = st->D, K = em->K, F = p->stft_size / 2 + 1;
    GSS_TRY(check_online_targets(ctx, what, targets, S, K, states, F, D));
    GSS_TRY(check_mvdr_online_holds(ctx, what, holds, S, F, D));
    GSS_TRY(check_stream_block_tail(ctx, what, p, cfg, st, wpe));
    const bool guided = act != nullptr;
    const int64_t Tn = gss_stream_num_frames(st->received, n, p->stft_size, p->stft_shift);
    const int64_t R = mvdr_online_lookahead_rows(holds, Tn);
    const int64_t after = std::min<int64_t>(holds[0].L, (int64_t)holds[0].held + Tn);
    const int64_t rows = R + (release ? after : 0);
    GSS_REQUIRE(ctx, (int64_t)S * (Tn + rows) < 2147483647, GSS_ERR_UNSUPPORTED,
                "%s: too many frames", what);
    if (samples_out)
        *samples_out = gss_stream_num_samples_out(st->frames_out * (int64_t)p->stft_shift,
                                                  rows * (int64_t)p->stft_shift, p->stft_size,
                                                  p->stft_shift);
    if (n == 0 && rows == 0) return GSS_OK;

    const bool masks = taps && (taps->target_mask || taps->distortion_mask);
    {
        size_t stage = stream_stft_workspace_bytes(Tn, D, guided ? K : 0, p->stft_size, p->stft_shift);
        Workspace ws;
        stream_lookahead_blocks(ws, p->wpe != 0, guided, masks, F, Tn, rows, D, K, S);
        if (Tn > 0) {
            if (p->wpe)
                stage = std::max(stage, wpe_online_workspace_bytes(F, Tn, wpe_arrays_of(p),
                                                                   D / wpe_arrays_of(p), p->wpe_taps,
                                                                   p->wpe_delay, false));
            stage = std::max(stage, cacgmm_online_workspace_bytes(F, K, D, false));
            stage = std::max(stage, mvdr_online_lookahead_workspace_bytes(F, S));
        }
        stage = std::max(stage, stream_istft_targets_workspace_bytes(rows, S, p->stft_size, p->stft_shift));
        GSS_TRY(arena_reserve(ctx, ws.bytes + 4096 + stage + (1 << 16)));
    }
    if (Tn > 0) ctx->last_online_targets = S;
    Workspace ws(ctx);
    const StreamBlockBuffers b =
        stream_lookahead_blocks(ws, p->wpe != 0, guided, masks, F, Tn, rows, D, K, S);
    GSS_TRY(ws.status(what));
    const size_t mark = ctx->arena_off;
    if (Tn == 0 && n > 0) {   // the samples enter the history, no frame is complete yet
        GSS_TRY(stream_stft_run(ctx, x, in_type, act, n, st, nullptr, nullptr));
        GSS_TRY(arena_release(ctx, mark));
    }
    if (Tn > 0) {
        GSS_TRY(stream_block_front(ctx, p, cfg, st, wpe, em, x, in_type, act, n, Tn, b, mark));
        const OnlineTargetStates bf(states, S);
        GSS_TRY(mvdr_online_lookahead_targets_run(ctx, b.X, F, Tn, D, b.gamma, K, targets, S,
                                                  /*ban=*/1, cfg->bf_forget, cfg->ref_channel,
                                                  bf.phi_x, bf.phi_n, holds, p->postfilter == 1, b.mx,
                                                  b.mn, b.Xhat, rows, nullptr, b.ref));
        GSS_TRY(arena_release(ctx, mark));
    }
    if (release)
        GSS_TRY(mvdr_online_release_run(ctx, holds, S, p->postfilter == 1,
                                        b.Xhat ? b.Xhat + (size_t)R * F : nullptr, rows, nullptr));
    if (rows > 0) GSS_TRY(stream_istft_targets_run(ctx, b.Xhat, rows, S, st, tails, out));
    if (taps) {
        const size_t ft = (size_t)F * Tn;
        if (Tn > 0) {
            GSS_TRY(copy_tap(ctx, taps->Obs_ftd, b.X, sizeof(cplx) * ft * D));
            if (guided) GSS_TRY(copy_tap(ctx, taps->act_frames, b.actf, (size_t)K * Tn));
            GSS_TRY(copy_tap(ctx, taps->gamma, b.gamma, sizeof(double) * ft * K));
            GSS_TRY(copy_tap(ctx, taps->target_mask, b.mx, sizeof(double) * ft * S));
            GSS_TRY(copy_tap(ctx, taps->distortion_mask, b.mn, sizeof(double) * ft * S));
            GSS_TRY(copy_tap(ctx, taps->ref_channel, b.ref, sizeof(int32_t) * S));
        }
        if (rows > 0) GSS_TRY(copy_tap(ctx, taps->Xhat, b.Xhat, sizeof(cplx) * F * rows * S));
    }
    return GSS_OK;
}
