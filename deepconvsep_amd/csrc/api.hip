// C-ABI entry points that are not tied to the network: context, framing integers, STFT plan,
// tiling.  (Network + fused path: net.hip.)
#include <math.h>
#include <stdarg.h>
#include <string.h>

#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "dcs_internal.h"

static thread_local char g_err[512] = "";

void dcs_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* dcs_last_error(void) { return g_err; }
extern "C" int dcs_version(void) { return 100; }

// ------------------------------------------------------------------------------- buffers / timing
namespace {
// a guarded block of dcs_dev_alloc: [red zone | bytes | padding to 256 | red zone], the padding checked as red zone
struct GuardedBlock {
    void* base;
    char* ptr;
    size_t bytes, guard_end;   // guard_end: bytes from ptr to the end of the allocation
    std::string name;
};
struct GuardRegistry {
    std::mutex mu;
    std::vector<DcsBuffer*> live;
    std::vector<GuardedBlock> owned;
};
GuardRegistry& guard_registry() {
    static GuardRegistry r;
    return r;
}
size_t guard_bytes_env() {
    static const size_t v = getenv("DCS_WS_GUARD") ? (size_t)atoll(getenv("DCS_WS_GUARD")) / 256 * 256 : 0;
    return v;
}
int guard_poison_env() {
    static const int v = getenv("DCS_WS_POISON") ? (atoi(getenv("DCS_WS_POISON")) & 0xff) : 0xff;
    return v;
}
}  // namespace

int DcsBuffer::ensure(size_t need) {
    if (need <= bytes) return DCS_OK;
    if (ptr) {
        // other work on the stream may still read the old block
        DCS_HIP(hipDeviceSynchronize());
        release();
    }
    const size_t want = need + need / 8;
    const size_t g = guard_bytes_env();
    if (g == 0) {
        DCS_HIP(hipMalloc(&ptr, want));
        base = ptr;
        bytes = want;
        return DCS_OK;
    }
    const size_t payload = (want + 255) / 256 * 256;
    DCS_HIP(hipMalloc(&base, payload + 2 * g));
    DCS_HIP(hipMemset(base, guard_poison_env(), payload + 2 * g));
    DCS_HIP(hipDeviceSynchronize());
    ptr = (char*)base + g;
    bytes = payload;
    guard = g;
    GuardRegistry& r = guard_registry();
    std::lock_guard<std::mutex> lk(r.mu);
    if (std::find(r.live.begin(), r.live.end(), this) == r.live.end()) r.live.push_back(this);
    return DCS_OK;
}

hipError_t dcs_dev_alloc(void** p, size_t bytes, const char* name) {
    *p = nullptr;
    const size_t g = guard_bytes_env();
    if (g == 0) return hipMalloc(p, bytes);
    const size_t payload = (bytes + 255) / 256 * 256;
    void* base = nullptr;
    hipError_t e = hipMalloc(&base, payload + 2 * g);
    if (e != hipSuccess) return e;
    if ((e = hipMemset(base, guard_poison_env(), payload + 2 * g)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) {
        (void)hipFree(base);
        return e;
    }
    char* ptr = (char*)base + g;
    GuardRegistry& r = guard_registry();
    std::lock_guard<std::mutex> lk(r.mu);
    r.owned.push_back(GuardedBlock{base, ptr, bytes, payload + g, name ? name : "?"});
    *p = ptr;
    return hipSuccess;
}

void dcs_dev_free(void* p) {
    if (!p) return;
    if (guard_bytes_env() != 0) {
        GuardRegistry& r = guard_registry();
        std::lock_guard<std::mutex> lk(r.mu);
        for (size_t i = 0; i < r.owned.size(); ++i)
            if (r.owned[i].ptr == p) {
                (void)hipFree(r.owned[i].base);
                r.owned.erase(r.owned.begin() + (std::ptrdiff_t)i);
                return;
            }
    }
    (void)hipFree(p);
}

void DcsBuffer::release() {
    if (base) (void)hipFree(base);
    else if (ptr) (void)hipFree(ptr);
    ptr = base = nullptr;
    bytes = guard = 0;
}

DcsBuffer::~DcsBuffer() {
    if (guard_bytes_env() == 0) return;
    GuardRegistry& r = guard_registry();
    std::lock_guard<std::mutex> lk(r.mu);
    r.live.erase(std::remove(r.live.begin(), r.live.end(), this), r.live.end());
}

long long dcs_buffers_check_guards(char* where, size_t where_len) {
    GuardRegistry& r = guard_registry();
    std::lock_guard<std::mutex> lk(r.mu);
    long long bad = 0;
    const unsigned char poison = (unsigned char)guard_poison_env();
    std::vector<unsigned char> h;
    // bytes [lo, hi) of the allocation around `ptr` (lo < 0: leading red zone) must still hold the poison
    auto check = [&](const char* ptr, std::ptrdiff_t lo, std::ptrdiff_t hi, size_t bytes, const char* what, const char* name) -> bool {
        h.resize((size_t)(hi - lo));
        if (hipMemcpy(h.data(), ptr + lo, h.size(), hipMemcpyDeviceToHost) != hipSuccess) return false;
        for (size_t i = 0; i < h.size(); ++i)
            if (h[i] != poison) {
                if (bad == 0 && where) {
                    const std::ptrdiff_t at = lo + (std::ptrdiff_t)i;
                    if (at < 0)
                        snprintf(where, where_len, "leading red zone of %s%s (%zu bytes), %td bytes before the block", what, name, bytes, -at);
                    else
                        snprintf(where, where_len, "trailing red zone of %s%s (%zu bytes), byte %td past the end of the block", what, name,
                                 bytes, at - (std::ptrdiff_t)bytes);
                }
                ++bad;
            }
        return true;
    };
    for (DcsBuffer* b : r.live) {
        if (!b->base || b->guard == 0) continue;
        const std::ptrdiff_t g = (std::ptrdiff_t)b->guard, n = (std::ptrdiff_t)b->bytes;
        if (!check((const char*)b->ptr, -g, 0, b->bytes, "a scratch block", "") ||
            !check((const char*)b->ptr, n, n + g, b->bytes, "a scratch block", ""))
            return -1;
    }
    const std::ptrdiff_t g = (std::ptrdiff_t)guard_bytes_env();
    for (const GuardedBlock& o : r.owned)
        if (!check(o.ptr, -g, 0, o.bytes, "", o.name.c_str()) ||
            !check(o.ptr, (std::ptrdiff_t)o.bytes, (std::ptrdiff_t)o.guard_end, o.bytes, "", o.name.c_str()))
            return -1;
    return bad;
}

extern "C" int dcs_debug_check_guards(dcs_ctx* ctx, int64_t* n_blocks_out) {
    if (!ctx) DCS_FAIL(DCS_EINVAL, "dcs_debug_check_guards: null context");
    if (guard_bytes_env() == 0)
        DCS_FAIL(DCS_EUNSUPPORTED, "dcs_debug_check_guards: the process was started without DCS_WS_GUARD=<bytes>");
    DCS_ON_DEVICE(ctx->device);
    DCS_HIP(hipDeviceSynchronize());
    if (n_blocks_out) {
        GuardRegistry& r = guard_registry();
        std::lock_guard<std::mutex> lk(r.mu);
        int64_t n = 0;
        for (DcsBuffer* b : r.live) n += (b->base && b->guard) ? 1 : 0;
        *n_blocks_out = n + (int64_t)r.owned.size();
    }
    char where[200] = "";
    const long long bad = dcs_buffers_check_guards(where, sizeof(where));
    if (bad < 0) DCS_FAIL(DCS_EHIP, "dcs_debug_check_guards: copying a red zone failed");
    if (bad > 0) DCS_FAIL(DCS_EHIP, "red zones damaged: %lld bytes, first in the %s", bad, where);
    return DCS_OK;
}

int DcsUploadRing::begin(size_t bytes, void** host_out, void** dev_out) {
    if (bytes == 0) bytes = 16;
    const int slot = (int)(next++ % kSlots);
    if (ev[slot]) DCS_HIP(hipEventSynchronize(ev[slot]));   // the upload that last used this slot has run (long ago, normally)
    else DCS_HIP(hipEventCreateWithFlags(&ev[slot], hipEventDisableTiming));
    if (cap[slot] < bytes) {
        if (host[slot]) DCS_HIP(hipHostFree(host[slot]));
        host[slot] = nullptr;
        cap[slot] = 0;
        const size_t want = bytes + bytes / 4 + 256;
        DCS_HIP(hipHostMalloc(&host[slot], want, hipHostMallocDefault));
        cap[slot] = want;
    }
    DCS_CHECK(dev.ensure(bytes));   // synchronises the device when (and only when) the block has to grow
    cur = slot;
    *host_out = host[slot];
    *dev_out = dev.ptr;
    return DCS_OK;
}

int DcsUploadRing::commit(size_t bytes, hipStream_t stream) {
    if (cur < 0) DCS_FAIL(DCS_EINVAL, "upload ring: commit without begin");
    if (bytes) DCS_HIP(hipMemcpyAsync(dev.ptr, host[cur], bytes, hipMemcpyHostToDevice, stream));
    DCS_HIP(hipEventRecord(ev[cur], stream));
    cur = -1;
    return DCS_OK;
}

void DcsUploadRing::release() {
    for (int i = 0; i < kSlots; ++i) {
        if (ev[i]) { (void)hipEventSynchronize(ev[i]); (void)hipEventDestroy(ev[i]); }
        if (host[i]) (void)hipHostFree(host[i]);
        ev[i] = nullptr; host[i] = nullptr; cap[i] = 0;
    }
    dev.release();
    cur = -1;
}

DcsTimer::DcsTimer(dcs_ctx* c, int t) : ctx(c), tag(t), idx(0), on(t >= 0 && ((c->timing_mask >> t) & 1u)) {   // t < 0: no-op
    if (!on) return;
    if ((c->timing_seen[t]++ % (uint64_t)c->timing_stride) != 0) {
        on = false;
        return;
    }
    DcsTimingSlot& s = ctx->slots[tag];
    if (s.used == s.start.size()) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
            on = false;
            return;
        }
        s.start.push_back(a);
        s.stop.push_back(b);
    }
    idx = s.used++;
    (void)hipEventRecord(s.start[idx], ctx->stream);
}

void DcsTimer::done() {
    if (on) (void)hipEventRecord(ctx->slots[tag].stop[idx], ctx->stream);
}

// nothing was launched after all: give the slot back (only valid while it is the tag's most recent one)
void DcsTimer::cancel() {
    if (!on) return;
    ctx->slots[tag].used = idx;
    on = false;
}

extern "C" int dcs_timing_enable(dcs_ctx* ctx, unsigned tag_mask) {
    if (!ctx) DCS_FAIL(DCS_EINVAL, "dcs_timing_enable: null ctx");
    ctx->timing_mask = tag_mask;
    return DCS_OK;
}

extern "C" int dcs_timing_stride(dcs_ctx* ctx, int stride) {
    if (!ctx || stride < 1) DCS_FAIL(DCS_EINVAL, "dcs_timing_stride: bad argument");
    ctx->timing_stride = stride;
    return DCS_OK;
}

extern "C" int dcs_timing_reset(dcs_ctx* ctx) {
    if (!ctx) DCS_FAIL(DCS_EINVAL, "dcs_timing_reset: null ctx");
    for (auto& s : ctx->slots) s.used = 0;
    for (auto& v : ctx->timing_seen) v = 0;
    return DCS_OK;
}

extern "C" int dcs_timing_query(dcs_ctx* ctx, int which, double* avg_ms, int64_t* launches) {
    if (!ctx || which < 0 || which >= DCS_TAG_COUNT) DCS_FAIL(DCS_EINVAL, "dcs_timing_query: bad argument");
    DCS_ON_DEVICE(ctx->device);
    DCS_HIP(hipStreamSynchronize(ctx->stream));
    DcsTimingSlot& s = ctx->slots[which];
    double total = 0.0;
    for (size_t i = 0; i < s.used; ++i) {
        float ms = 0.f;
        DCS_HIP(hipEventElapsedTime(&ms, s.start[i], s.stop[i]));
        total += ms;
    }
    if (avg_ms) *avg_ms = s.used ? total / (double)s.used : 0.0;
    if (launches) *launches = (int64_t)s.used;
    return DCS_OK;
}

// ------------------------------------------------------------------------------- context
extern "C" int dcs_create(int device, void* hip_stream, dcs_ctx** out) {
    if (!out) DCS_FAIL(DCS_EINVAL, "dcs_create: out is null");
    int count = 0;
    DCS_HIP(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) DCS_FAIL(DCS_EINVAL, "dcs_create: device %d of %d", device, count);
    DCS_ON_DEVICE(device);   // the caller's current device is restored on return
    hipDeviceProp_t prop;
    DCS_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        DCS_FAIL(DCS_EUNSUPPORTED, "dcs_create: device %d is %s; libdcs is built for gfx950 only", device,
                 prop.gcnArchName);
    dcs_ctx* c = new dcs_ctx();
    c->device = device;
    c->stream = reinterpret_cast<hipStream_t>(hip_stream);
    c->n_cu = prop.multiProcessorCount;
    *out = c;
    return DCS_OK;
}

extern "C" int dcs_destroy(dcs_ctx* ctx) {
    if (!ctx) return DCS_OK;
    DCS_ON_DEVICE(ctx->device);
    for (auto& s : ctx->slots) {
        for (auto e : s.start) (void)hipEventDestroy(e);
        for (auto e : s.stop) (void)hipEventDestroy(e);
    }
    ctx->gemm_ws.release();
    ctx->bss_ws.release();
    ctx->mwf_ws.release();
    ctx->align_ws.release();
    ctx->score_ring.release();
    dcs_dev_free(ctx->ola_rise_d);
    delete ctx;
    return DCS_OK;
}


extern "C" int dcs_synchronize(dcs_ctx* ctx) {
    if (!ctx) DCS_FAIL(DCS_EINVAL, "dcs_synchronize: null ctx");
    DCS_ON_DEVICE(ctx->device);
    DCS_HIP(hipStreamSynchronize(ctx->stream));
    return DCS_OK;
}

// ------------------------------------------------------------------------------- framing integers
extern "C" int64_t dcs_frame_count(int64_t n_samples, int hop) {
    if (hop <= 0 || n_samples < 0) return -1;
    // int(np.ceil(lengthData / np.double(hopsize)) + 2)        transform.py:309
    return (n_samples + hop - 1) / hop + 2;
}

extern "C" int64_t dcs_inverse_length(int64_t n_frames, int hop, int frame) {
    if (n_frames <= 0 || hop <= 0 || frame <= 0) return -1;
    // int(hopsize*(numberFrames-1) + lengthWindow) - int(lengthWindow/2.0)   transform.py:373,390
    return (int64_t)hop * (n_frames - 1) + frame - frame / 2;
}

extern "C" int64_t dcs_tile_count(int64_t n_frames, int tc, int ov, int tiler) {
    if (tc <= 0 || ov < 0 || ov >= tc) return -1;
    const int64_t guard = (tiler == DCS_TILER_SCRIPT) ? tc : ov;
    const int64_t stride = tc - ov;
    // tiles while start + guard < T, start = i * stride
    if (n_frames <= guard) return 0;
    return (n_frames - guard - 1) / stride + 1;
}

// ------------------------------------------------------------------------------- STFT plan
extern "C" int dcs_stft_plan(dcs_ctx* ctx, int frame, int hop, const double* window_h, dcs_stft** out) {
    if (!ctx || !window_h || !out) DCS_FAIL(DCS_EINVAL, "dcs_stft_plan: null argument");
    if (frame < 16 || frame > 8192 || (frame & (frame - 1)))
        DCS_FAIL(DCS_EUNSUPPORTED, "dcs_stft_plan: frameSize %d is not a power of two in [16, 8192]", frame);
    if (hop <= 0 || hop > frame) DCS_FAIL(DCS_EINVAL, "dcs_stft_plan: hopSize %d not in (0, %d]", hop, frame);
    DCS_ON_DEVICE(ctx->device);
    dcs_stft* p = new dcs_stft();
    p->ctx = ctx;
    p->frame = frame;
    p->hop = hop;
    int M = frame / 2, lg = 0;
    while ((1 << lg) < M) ++lg;
    p->log2m = lg;

    std::vector<float> wf(frame), wsqf(frame);
    std::vector<double> wsqd(frame);
    for (int i = 0; i < frame; ++i) {
        wf[i] = (float)window_h[i];
        wsqd[i] = window_h[i] * window_h[i];
        wsqf[i] = (float)wsqd[i];
    }
    std::vector<double2> twd(M + 1);
    std::vector<float2> twf(M + 1);
    const double pi = 3.14159265358979323846;
    for (int k = 0; k <= M; ++k) {
        double a = -2.0 * pi * (double)k / (double)frame;
        twd[k].x = cos(a);
        twd[k].y = sin(a);
    }
    // exact values on the axes (keeps DC / Nyquist bins exactly real like numpy's rfft)
    twd[0].x = 1.0; twd[0].y = 0.0;
    twd[M].x = -1.0; twd[M].y = 0.0;
    if (M % 2 == 0) { twd[M / 2].x = 0.0; twd[M / 2].y = -1.0; }
    for (int k = 0; k <= M; ++k) {
        twf[k].x = (float)twd[k].x;
        twf[k].y = (float)twd[k].y;
    }
    auto up = [&](void** dst, const void* src, size_t bytes, const char* name) -> int {
        DCS_HIP(dcs_dev_alloc(dst, bytes, name));
        DCS_HIP(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
        return DCS_OK;
    };
    int rc = DCS_OK;
    if ((rc = up((void**)&p->win_f, wf.data(), frame * sizeof(float), "stft.win_f")) ||
        (rc = up((void**)&p->win_d, window_h, frame * sizeof(double), "stft.win_d")) ||
        (rc = up((void**)&p->wsq_f, wsqf.data(), frame * sizeof(float), "stft.wsq_f")) ||
        (rc = up((void**)&p->wsq_d, wsqd.data(), frame * sizeof(double), "stft.wsq_d")) ||
        (rc = up((void**)&p->tw_f, twf.data(), (M + 1) * sizeof(float2), "stft.tw_f")) ||
        (rc = up((void**)&p->tw_d, twd.data(), (M + 1) * sizeof(double2), "stft.tw_d"))) {
        dcs_stft_plan_destroy(p);
        return rc;
    }
    *out = p;
    return DCS_OK;
}

extern "C" int dcs_stft_plan_destroy(dcs_stft* p) {
    if (!p) return DCS_OK;
    DCS_ON_DEVICE(p->ctx->device);
    dcs_dev_free(p->win_f);
    dcs_dev_free(p->win_d);
    dcs_dev_free(p->wsq_f);
    dcs_dev_free(p->wsq_d);
    dcs_dev_free(p->tw_f);
    dcs_dev_free(p->tw_d);
    delete p;
    return DCS_OK;
}

template <typename R, typename R2>
static int forward_checked(dcs_stft* p, const R* audio, int64_t L, R* mag, R* phase, int64_t ld, int64_t rows_out,
                           int (*launch)(dcs_stft*, const R*, int64_t, R*, R*, R2*, int64_t, int64_t, int64_t)) {
    if (!p || !mag || (!audio && L > 0)) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward: null argument");
    if (L < 0) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward: negative length");
    DCS_ON_DEVICE(p->ctx->device);
    const int64_t T = dcs_frame_count(L, p->hop);
    if (ld < p->frame / 2 + 1) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward: ld %lld < bins %d", (long long)ld, p->frame / 2 + 1);
    if (rows_out < T) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward: rows_out %lld < frames %lld", (long long)rows_out, (long long)T);
    return launch(p, audio, L, mag, phase, (R2*)nullptr, ld, rows_out, T);
}

extern "C" int dcs_stft_forward_f32(dcs_stft* p, const float* audio_d, int64_t n, float* mag_d, float* phase_d,
                                    int64_t ld, int64_t rows_out) {
    return forward_checked<float, float2>(p, audio_d, n, mag_d, phase_d, ld, rows_out, dcs_launch_stft_forward_f32);
}
extern "C" int dcs_stft_forward_f64(dcs_stft* p, const double* audio_d, int64_t n, double* mag_d, double* phase_d,
                                    int64_t ld, int64_t rows_out) {
    return forward_checked<double, double2>(p, audio_d, n, mag_d, phase_d, ld, rows_out, dcs_launch_stft_forward_f64);
}

// compute_transform (transform.py:80-131): every column of audio[t, i] -- n_clips signals of equal length -- in ONE launch
static int forward_clips_check(dcs_stft* p, const void* audio, int64_t L, int64_t n_clips, int64_t clip_stride, const void* mag,
                               int64_t ld, int64_t rows_out, int64_t* T) {
    if (!p || !mag || (!audio && L > 0)) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_clips: null argument");
    if (L < 0 || n_clips < 0) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_clips: negative size");
    if (n_clips > 1 && clip_stride < L) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_clips: clip stride %lld < length %lld", (long long)clip_stride, (long long)L);
    *T = dcs_frame_count(L, p->hop);
    if (ld < p->frame / 2 + 1) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward: ld %lld < bins %d", (long long)ld, p->frame / 2 + 1);
    if (rows_out < *T) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward: rows_out %lld < frames %lld", (long long)rows_out, (long long)*T);
    if (rows_out * n_clips > 0x7fffffffLL) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_clips: %lld rows in one launch", (long long)(rows_out * n_clips));
    return DCS_OK;
}
extern "C" int dcs_stft_forward_f32_clips(dcs_stft* p, const float* audio_d, int64_t n, int64_t n_clips, int64_t clip_stride,
                                          float* mag_d, float* phase_d, int64_t ld, int64_t rows_out) {
    int64_t T = 0;
    DCS_CHECK(forward_clips_check(p, audio_d, n, n_clips, clip_stride, mag_d, ld, rows_out, &T));
    if (n_clips == 0) return DCS_OK;
    DCS_ON_DEVICE(p->ctx->device);
    return dcs_launch_stft_forward_f32_clips(p, audio_d, n, clip_stride, n_clips, mag_d, phase_d, nullptr, ld, rows_out, T, false);
}
extern "C" int dcs_stft_forward_f64_clips(dcs_stft* p, const double* audio_d, int64_t n, int64_t n_clips, int64_t clip_stride,
                                          double* mag_d, double* phase_d, int64_t ld, int64_t rows_out) {
    int64_t T = 0;
    DCS_CHECK(forward_clips_check(p, audio_d, n, n_clips, clip_stride, mag_d, ld, rows_out, &T));
    if (n_clips == 0) return DCS_OK;
    DCS_ON_DEVICE(p->ctx->device);
    return dcs_launch_stft_forward_f64_clips(p, audio_d, n, clip_stride, n_clips, mag_d, phase_d, ld, rows_out, T);
}

template <typename R, typename R2>
static int inverse_checked(dcs_stft* p, const R* mag, int64_t src_stride, const R* phase, int64_t ld, int64_t T,
                           int n_src, R pre_div, R* audio, int64_t n_out,
                           int (*launch)(dcs_stft*, const R*, int64_t, const R*, const R2*, int64_t, int64_t, int, R, R*,
                                         int64_t)) {
    if (!p || !mag || !phase || !audio) DCS_FAIL(DCS_EINVAL, "dcs_stft_inverse: null argument");
    if (T <= 0 || n_src <= 0) DCS_FAIL(DCS_EINVAL, "dcs_stft_inverse: empty input");
    DCS_ON_DEVICE(p->ctx->device);
    if (ld < p->frame / 2 + 1) DCS_FAIL(DCS_EINVAL, "dcs_stft_inverse: ld < bins");
    if (n_out < 0 || n_out > dcs_inverse_length(T, p->hop, p->frame))
        DCS_FAIL(DCS_EINVAL, "dcs_stft_inverse: n_out %lld exceeds %lld", (long long)n_out,
                 (long long)dcs_inverse_length(T, p->hop, p->frame));
    if (pre_div == R(0)) DCS_FAIL(DCS_EINVAL, "dcs_stft_inverse: pre_div is zero");
    return launch(p, mag, src_stride, phase, (const R2*)nullptr, ld, T, n_src, pre_div, audio, n_out);
}

extern "C" int dcs_stft_inverse_f32(dcs_stft* p, const float* mag_d, int64_t src_stride, const float* phase_d,
                                    int64_t ld, int64_t T, int n_src, float pre_div, float* audio_d, int64_t n_out) {
    return inverse_checked<float, float2>(p, mag_d, src_stride, phase_d, ld, T, n_src, pre_div, audio_d, n_out,
                                  dcs_launch_stft_inverse_f32);
}
extern "C" int dcs_stft_inverse_f64(dcs_stft* p, const double* mag_d, int64_t src_stride, const double* phase_d,
                                    int64_t ld, int64_t T, int n_src, double pre_div, double* audio_d,
                                    int64_t n_out) {
    return inverse_checked<double, double2>(p, mag_d, src_stride, phase_d, ld, T, n_src, pre_div, audio_d, n_out,
                                   dcs_launch_stft_inverse_f64);
}

// ------------------------------------------------------------------------------- test aids for the transform kernels
// the device clip table on the host, checked against the rows / samples the caller's arguments describe
static int debug_clip_table(dcs_stft* p, const int64_t* clip_tab_d, int64_t n_clips, std::vector<int64_t>* tab) {
    tab->resize((size_t)n_clips * kDcsClipTab);
    DCS_HIP(hipStreamSynchronize(p->ctx->stream));
    DCS_HIP(hipMemcpy(tab->data(), clip_tab_d, tab->size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    int compact = 0;
    for (int64_t c = 0; c < n_clips; ++c) compact += (*tab)[c * kDcsClipTab + 3] >= 0;
    if (compact != 0 && compact != n_clips) DCS_FAIL(DCS_EINVAL, "clip table: row offsets in some clips only");
    return DCS_OK;
}

extern "C" int dcs_debug_stft_forward_f32(dcs_stft* p, const float* audio_d, int64_t n, int64_t audio_stride, int64_t n_clips,
                                          float* mag_d, float* phase_d, float* unit_d, int64_t ld, int64_t rows_out,
                                          int interleave, const int64_t* clip_tab_d) {
    int64_t T = 0;
    if (rows_out < 0) DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_forward: negative size");
    if (!audio_d) DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_forward: null argument");
    DCS_CHECK(forward_clips_check(p, audio_d, n, n_clips, audio_stride, mag_d, ld, rows_out, &T));
    if (n_clips == 0) return DCS_OK;
    if (clip_tab_d && interleave) DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_forward: a clip table with interleaved rows");
    DCS_ON_DEVICE(p->ctx->device);
    if (clip_tab_d) {
        std::vector<int64_t> tab;
        DCS_CHECK(debug_clip_table(p, clip_tab_d, n_clips, &tab));
        for (int64_t c = 0; c < n_clips; ++c) {
            const int64_t* e = &tab[c * kDcsClipTab];
            if (e[0] < 0 || e[0] > n || e[1] != dcs_frame_count(e[0], p->hop) || e[1] > rows_out)
                DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_forward: clip %lld of the table: %lld samples, %lld frames", (long long)c,
                         (long long)e[0], (long long)e[1]);
            if (e[3] >= 0 && (e[5] < e[1] || e[5] > rows_out || e[3] > rows_out * n_clips - e[5]))
                DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_forward: clip %lld of the table: rows [%lld, +%lld) of %lld", (long long)c,
                         (long long)e[3], (long long)e[5], (long long)(rows_out * n_clips));
        }
    }
    return dcs_launch_stft_forward_f32_clips(p, audio_d, n, audio_stride, n_clips, mag_d, phase_d,
                                             reinterpret_cast<float2*>(unit_d), ld, rows_out, T, interleave != 0, clip_tab_d);
}

extern "C" int dcs_debug_stft_inverse_unit_f32(dcs_stft* p, const float* mag_d, int64_t src_stride, const float* unit_d,
                                               int64_t unit_clip_stride, int64_t ld, int64_t T, int n_src, int64_t n_clips,
                                               float pre_div, float* audio_d, int64_t n_out, const int64_t* clip_tab_d,
                                               int64_t out_stride) {
    if (!p || !mag_d || !unit_d || !audio_d) DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_inverse_unit: null argument");
    if (T < 0 || n_src < 0 || n_clips < 0 || n_out < 0 || out_stride < 0)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_inverse_unit: negative size");
    if (ld < p->frame / 2 + 1) DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_inverse_unit: ld < bins");
    if (!(pre_div != 0.f) || !std::isfinite(pre_div)) DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_inverse_unit: pre_div");
    if (out_stride != 0 && out_stride < n_out) DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_inverse_unit: out_stride < n_out");
    if (T > 0x7fffffffLL / ld) DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_inverse_unit: %lld frames", (long long)T);
    if (n_clips > 1 && unit_clip_stride < T * ld) DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_inverse_unit: unit_clip_stride < n_frames * ld");
    if (n_src * n_clips > 1 && src_stride < T * ld) DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_inverse_unit: src_stride < n_frames * ld");
    if (n_src * n_clips > 0x7fffLL) DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_inverse_unit: %lld sources", (long long)(n_src * n_clips));
    if (T == 0 || n_src == 0 || n_clips == 0 || n_out == 0) return DCS_OK;
    if (n_out > dcs_inverse_length(T, p->hop, p->frame))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_inverse_unit: n_out %lld exceeds %lld", (long long)n_out,
                 (long long)dcs_inverse_length(T, p->hop, p->frame));
    DCS_ON_DEVICE(p->ctx->device);
    if (clip_tab_d) {
        if (!dcs_stft_inverse_is_wave(p))
            DCS_FAIL(DCS_EUNSUPPORTED, "clips of different lengths need the wave iSTFT kernel (frameSize 1024 / 2048 / 4096, hop | frameSize)");
        std::vector<int64_t> tab;
        DCS_CHECK(debug_clip_table(p, clip_tab_d, n_clips, &tab));
        const int64_t unit_rows = ((n_clips - 1) * unit_clip_stride) / ld + T;   // what the strides describe
        for (int64_t c = 0; c < n_clips; ++c) {
            const int64_t* e = &tab[c * kDcsClipTab];
            if (e[0] < 0 || e[0] > n_out || e[1] < 0 || e[1] > T || (e[3] >= 0 && e[3] > unit_rows - e[1]))
                DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_inverse_unit: clip %lld of the table: %lld samples, %lld frames at row %lld",
                         (long long)c, (long long)e[0], (long long)e[1], (long long)e[3]);
        }
    }
    return dcs_launch_stft_inverse_f32_clips(p, mag_d, src_stride, reinterpret_cast<const float2*>(unit_d), unit_clip_stride, ld,
                                             T, n_src, n_clips, pre_div, audio_d, n_out, clip_tab_d, out_stride);
}

extern "C" int dcs_debug_stft_last_kernel(const dcs_stft* p, int* forward, int* inverse, int64_t* param) {
    if (!p) DCS_FAIL(DCS_EINVAL, "dcs_debug_stft_last_kernel: null plan");
    if (forward) *forward = p->last_fwd;
    if (inverse) *inverse = p->last_inv;
    if (param) *param = p->last_param;
    return DCS_OK;
}

// ------------------------------------------------------------------------------- tiling
extern "C" int dcs_tile(dcs_ctx* ctx, const float* mag_d, int64_t ch_stride, int64_t ld, int C, int64_t T, int F,
                        int tc, int ov, int tiler, float scale, float* tiles_d, int64_t n_tiles) {
    if (!ctx || !mag_d || (!tiles_d && n_tiles > 0)) DCS_FAIL(DCS_EINVAL, "dcs_tile: null argument");
    if (C < 1 || F < 1 || ld < F || tc < 1 || ov < 0 || ov >= tc) DCS_FAIL(DCS_EINVAL, "dcs_tile: bad shape");
    if (tiler != DCS_TILER_SCRIPT && tiler != DCS_TILER_LIBRARY) DCS_FAIL(DCS_EINVAL, "dcs_tile: bad tiler");
    if (tiler == DCS_TILER_SCRIPT && C != 1)
        DCS_FAIL(DCS_EINVAL, "dcs_tile: the script tiler takes a [T,F] spectrogram (separate_dsd.py:119)");
    if (n_tiles != dcs_tile_count(T, tc, ov, tiler))
        DCS_FAIL(DCS_EINVAL, "dcs_tile: n_tiles %lld != %lld", (long long)n_tiles,
                 (long long)dcs_tile_count(T, tc, ov, tiler));
    if (n_tiles == 0) return DCS_OK;
    DCS_ON_DEVICE(ctx->device);
    return dcs_launch_tile(ctx, mag_d, ch_stride, ld, C, T, F, tc, ov, tiler, scale, tiles_d, n_tiles);
}

extern "C" int dcs_overlap_add(dcs_ctx* ctx, const float* out_d, int64_t n, int S, int tc, int ov, int F,
                               const double* rise_h, float* sep_d, int64_t sep_stride, int64_t ld) {
    if (!ctx || !out_d || !sep_d || (!rise_h && ov > 0)) DCS_FAIL(DCS_EINVAL, "dcs_overlap_add: null argument");
    // overlap == 0 is legal in the reference (util.py:306-325 with an empty ramp): the tiles are laid end to end
    if (n < 0 || S < 1 || tc < 1 || ov < 0 || ov >= tc || F < 1 || ld < F)
        DCS_FAIL(DCS_EINVAL, "dcs_overlap_add: bad shape");
    if (ov > 256) DCS_FAIL(DCS_EUNSUPPORTED, "dcs_overlap_add: overlap > 256");
    DCS_ON_DEVICE(ctx->device);
    DCS_CHECK(dcs_ctx_ola_rise(ctx, rise_h, ov));
    return dcs_launch_overlap_add(ctx, out_d, n, S, tc, ov, F, ctx->ola_rise_d, sep_d, sep_stride, ld);
}

// the context's cross-fade ramp (ctx->ola_rise_d) holds rise_h[0 .. ov) as float32 on return: uploaded when the values change
int dcs_ctx_ola_rise(dcs_ctx* ctx, const double* rise_h, int ov) {
    std::vector<float> rise(ov);
    for (int i = 0; i < ov; ++i) rise[i] = (float)rise_h[i];
    if (ov > 0 && (rise != ctx->ola_rise_h || !ctx->ola_rise_d)) {
        // a new ramp: earlier launches on the stream may still read the old table
        DCS_HIP(hipStreamSynchronize(ctx->stream));
        dcs_dev_free(ctx->ola_rise_d);
        ctx->ola_rise_d = nullptr;
        ctx->ola_rise_h.clear();
        DCS_HIP(dcs_dev_alloc((void**)&ctx->ola_rise_d, ov * sizeof(float), "ctx.ola_rise"));
        DCS_HIP(hipMemcpy(ctx->ola_rise_d, rise.data(), ov * sizeof(float), hipMemcpyHostToDevice));
        ctx->ola_rise_h = rise;
    }
    return DCS_OK;
}
