// ovl_ctx.cpp — contexts and devices of the C ABI (ovl_ctx.h): error text, environment knobs, device setup and
// teardown, staging and pinned host memory, and the entry points that create, destroy and query a context.
#include "ovl_ctx.h"

thread_local std::string g_err;

int fail(const ovl_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    if (c) const_cast<ovl_ctx*>(c)->err = buf;
    return code;
}

int fail(const Dev* d, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    if (d && d->owner) d->owner->err = buf;
    return code;
}

void free_staging(int32_t*& p) {
    if (p) (void)hipHostFree(p);
    p = nullptr;
}

hipError_t alloc_staging(int32_t*& p, int32_t*& p_dev, int64_t cap) {
    hipError_t e = hipHostMalloc((void**)&p, (size_t)kSlots * 2 * (size_t)cap * sizeof(int32_t), kHostShared);
    if (e != hipSuccess) return e;
    return hipHostGetDevicePointer((void**)&p_dev, p, 0);
}

// True when [p, p + bytes) is pinned host memory (hipHostMalloc'd or registered), so DMA can
// read or write it in place.  hipPointerGetAttributes fails (or reports "unregistered") for
// pageable memory; its sticky error is cleared so later hipGetLastError callers (torch) see none.
bool host_pinned(const void* p, size_t bytes) {
    if (!p || bytes == 0) return false;
    const char* ends[2] = {(const char*)p, (const char*)p + bytes - 1};
    for (const char* q : ends) {
        hipPointerAttribute_t at;
        memset(&at, 0, sizeof(at));
        if (hipPointerGetAttributes(&at, q) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        if (at.type != hipMemoryTypeHost) return false;
    }
    return true;
}

// Stops the context's resident grids (ovl_resident.h) before other work on its devices: a grid's stream would hold
// a device synchronisation or a free until its idle deadline, and its blocks hold CU slots during other launches.
void quiet(ovl_ctx* c) {
    if (c)
        for (Dev* d : c->devs) (void)d->res.stop();
}

// ----------------------------------------------------------------------------- devices

namespace {

Knobs read_knobs() {
    Knobs k;
    if (const char* e = getenv("OVL_BAND_FORM")) {
        if (!strcmp(e, "diag")) k.band_form = OVL_BAND_FORM_DIAG;
        else if (!strcmp(e, "rows")) k.band_form = OVL_BAND_FORM_ROWS;
        else if (!strcmp(e, "fast")) k.band_form = OVL_BAND_FORM_FAST;
        else if (!strcmp(e, "strip")) k.band_form = OVL_BAND_FORM_STRIP;
        else if (!strcmp(e, "lane")) k.band_form = OVL_BAND_FORM_LANE;
        else if (!strcmp(e, "lane1")) k.band_form = OVL_BAND_FORM_LANE1;
        else if (!strcmp(e, "lane2")) k.band_form = OVL_BAND_FORM_LANE2;
    }
    if (const char* e = getenv("OVL_DP_FORM")) {
        if (!strcmp(e, "lane")) k.dp_lane = 1;
        else if (!strcmp(e, "fast")) k.dp_lane = 0;
        else if (!strcmp(e, "classic")) k.dp_classic = 1;
    }
    if (const char* e = getenv("OVL_LANE_FORM")) {
        const int v = atoi(e);
        k.lane_prof = v & 1;
        k.lane_sfx = (v >> 1) & 1;
        k.lane_h2 = (v >> 2) & 1;
    }
    if (const char* e = getenv("OVL_PACK")) k.pack = std::max(0, std::min(1, atoi(e)));
    if (const char* e = getenv("OVL_RESIDENT")) {  // mode[,blocks/CU[,pipelined[,poll sleep[,ring]]]] ("1x2x1x4x1")
        k.resident = std::max(0, std::min(2, atoi(e)));
        if (const char* c = strpbrk(e, ",x")) {
            k.resident_blocks = std::max(1, std::min(8, atoi(c + 1)));
            if (const char* c2 = strpbrk(c + 1, ",x")) {
                k.resident_pf = atoi(c2 + 1) != 0;
                if (const char* c3 = strpbrk(c2 + 1, ",x")) {
                    k.resident_sleep = std::max(0, std::min(1000, atoi(c3 + 1)));
                    if (const char* c4 = strpbrk(c3 + 1, ",x")) k.resident_ring = std::min(2, std::max(0, atoi(c4 + 1)));
                }
            }
        }
    }
    if (const char* e = getenv("OVL_PACK_MIN")) k.pack_min = std::max(0LL, atoll(e));
    if (const char* e = getenv("OVL_PACK_DIRECT_PCT")) {
        k.pack_direct_pct = std::max(0, std::min(100, atoi(e)));
        k.pack_adapt = 0;  // a fixed share
    }
    if (const char* e = getenv("OVL_PAIRS_FORM")) {
        if (!strcmp(e, "plain")) k.compact = 0;
        else if (!strcmp(e, "decode")) k.pairs_ix = 0;
    }
    if (const char* e = getenv("OVL_LOCAL_BATCH_WAVES")) k.local_batch_waves = std::max(0, atoi(e));
    if (const char* e = getenv("OVL_TR_WINDOW")) k.tr_window = std::max(0, atoi(e));
    if (const char* e = getenv("OVL_SEED_GROUPS")) k.seed_keep = strcmp(e, "search") != 0;
    if (const char* e = getenv("OVL_REACH_WINDOW")) k.reach_window = std::max(0, atoi(e));
    if (const char* e = getenv("OVL_READ_BEST_CHUNK")) k.read_best_chunk = std::max(0, atoi(e));
    if (const char* e = getenv("OVL_CONSENSUS_CHUNK")) k.consensus_chunk = std::max(0, atoi(e));
    if (const char* e = getenv("OVL_LAYOUT_LINK")) k.layout_runs = strcmp(e, "plain") != 0;
    if (const char* e = getenv("OVL_SPECTRUM_VOTE")) k.spec_ballot = strcmp(e, "ballot") == 0;
    if (const char* e = getenv("OVL_SPECTRUM_BINS")) k.spec_bins = std::min(std::max(atoi(e), 4), 1024);
    if (const char* e = getenv("OVL_PIPE_CHUNK")) {
        const long long v = atoll(e);
        if (v >= 64) k.pipe_chunk = v;
    }
    return k;
}

void destroy_dev(Dev* d) {
    if (!d) return;
    d->worker.reset();
    d->res.release();
    (void)hipSetDevice(d->device);
    for (hipStream_t s : {d->stream, d->s_in})
        if (s) (void)hipStreamSynchronize(s);
    if (d->l_tb_host) (void)hipHostFree(d->l_tb_host);
    free_staging(d->st_in);
    free_staging(d->st_out);
    if (d->h_flag) (void)hipHostFree(d->h_flag);
    if (d->cp_host) (void)hipHostFree(d->cp_host);
    for (hipEvent_t e : d->dec_ev)
        if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < kSlots; ++i)
        if (d->ev_k[i]) (void)hipEventDestroy(d->ev_k[i]);
    for (hipEvent_t e : d->t_ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : d->k_ev)
        if (e) (void)hipEventDestroy(e);
    if (d->scratch_evt) (void)hipEventDestroy(d->scratch_evt);
    if (d->ev_last) (void)hipEventDestroy(d->ev_last);
    for (hipStream_t s : {d->stream, d->s_in})
        if (s) (void)hipStreamDestroy(s);
    delete d;  // every DevBuf and every stage's timer goes here, with the device still current
}

hipError_t init_dev(Dev* d) {
    hipError_t e = hipSetDevice(d->device);
    if (e != hipSuccess) return e;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, d->device) == hipSuccess && prop.multiProcessorCount > 0)
        d->cu_count = prop.multiProcessorCount;
    d->res.device = d->device;
    d->res.cu_count = d->cu_count;
    d->res.blocks_per_cu = d->k.resident_blocks;
    d->res.pipelined = d->k.resident_pf;
    d->res.poll_sleep = d->k.resident_sleep;
    d->res.ring_kind = d->k.resident_ring;
    for (hipStream_t* s : {&d->stream, &d->s_in}) {
        e = hipStreamCreateWithFlags(s, hipStreamNonBlocking);
        if (e != hipSuccess) return e;
    }
    for (int i = 0; i < kSlots; ++i) {
        e = hipEventCreateWithFlags(&d->ev_k[i], hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    e = hipEventCreateWithFlags(&d->scratch_evt, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    e = hipEventCreateWithFlags(&d->ev_last, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    e = hipHostMalloc((void**)&d->h_flag, 64, kHostShared);
    if (e != hipSuccess) return e;
    *d->h_flag = 0;
    e = hipHostGetDevicePointer((void**)&d->h_flag_dev, d->h_flag, 0);
    if (e != hipSuccess) return e;
    e = ensure(d->err_flag, 16);
    if (e != hipSuccess) return e;
    return hipMemset(d->err_flag.p, 0, 16);
}

int create_on(const int32_t* ids, int32_t n, ovl_ctx** out) {
    int count = 0;
    HIPCHK((ovl_ctx*)nullptr, hipGetDeviceCount(&count));
    if (count <= 0) return fail((ovl_ctx*)nullptr, OVL_E_HIP, "no HIP device visible");
    if (n <= 0) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "no devices requested");
    // OVL_SHARE_DEVICES=1 (tests on a one-GPU box): a device may be listed more than once; each entry is
    // an independent shard slot (own streams, buffers, staging and flag) on that GPU, so the N-device
    // sharding, per-device jobs and slice copies run for real
    const char* share = getenv("OVL_SHARE_DEVICES");
    const bool allow_dup = share && atoi(share) == 1;
    for (int32_t i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= count)
            return fail((ovl_ctx*)nullptr, OVL_E_ARG, "device %d outside [0, %d)", ids[i], count);
        for (int32_t j = 0; j < i && !allow_dup; ++j)
            if (ids[j] == ids[i]) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "device %d listed twice", ids[i]);
    }
    DeviceGuard guard;
    CpuShare::get().refresh(true);
    ovl_ctx* c = new ovl_ctx();
    c->shared_slots = allow_dup;
    const Knobs knobs = read_knobs();
    for (int32_t i = 0; i < n; ++i) {
        Dev* d = new Dev();
        d->owner = c;
        d->device = ids[i];
        d->k = knobs;
        c->devs.push_back(d);
        hipError_t e = init_dev(d);
        if (e != hipSuccess) {
            int rc = fail((ovl_ctx*)nullptr, e == hipErrorOutOfMemory ? OVL_E_OOM : OVL_E_HIP,
                          "context setup on device %d: %s", ids[i], hipGetErrorString(e));
            ovl_destroy(c);
            return rc;
        }
    }
    *out = c;
    return OVL_OK;
}

}  // namespace

// ----------------------------------------------------------------------------- context

OVL_API int ovl_version(void) { return OVL_ABI_VERSION; }

OVL_API const char* ovl_last_error(const ovl_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

OVL_API int ovl_device_count(int32_t* out_count) {
    if (!out_count) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "out_count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *out_count = 0;
        return fail((ovl_ctx*)nullptr, OVL_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *out_count = n;
    return OVL_OK;
}

OVL_API int ovl_create(int32_t n_devices, ovl_ctx** out_ctx) {
    if (!out_ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "out_ctx is NULL");
    *out_ctx = nullptr;
    if (n_devices < 0) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "n_devices < 0 (0 = all visible devices)");
    int count = 0, cur = 0;
    HIPCHK((ovl_ctx*)nullptr, hipGetDeviceCount(&count));
    if (count <= 0) return fail((ovl_ctx*)nullptr, OVL_E_HIP, "no HIP device visible");
    if (n_devices == 0) n_devices = count;
    if (n_devices > count)
        return fail((ovl_ctx*)nullptr, OVL_E_ARG, "n_devices %d > visible devices %d", n_devices, count);
    HIPCHK((ovl_ctx*)nullptr, hipGetDevice(&cur));
    std::vector<int32_t> ids((size_t)n_devices);
    for (int32_t i = 0; i < n_devices; ++i) ids[(size_t)i] = (cur + i) % count;
    return create_on(ids.data(), n_devices, out_ctx);
}

OVL_API int ovl_create_on_devices(const int32_t* devices, int32_t n_devices, ovl_ctx** out_ctx) {
    if (!out_ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "out_ctx is NULL");
    *out_ctx = nullptr;
    if (!devices || n_devices <= 0) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "empty device list");
    return create_on(devices, n_devices, out_ctx);
}

OVL_API int ovl_ctx_devices(const ovl_ctx* c, int32_t* ids, int32_t cap, int32_t* out_n) {
    if (!c) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    if (out_n) *out_n = (int32_t)c->devs.size();
    for (int32_t i = 0; ids && i < cap && i < (int32_t)c->devs.size(); ++i) ids[i] = c->devs[(size_t)i]->device;
    return OVL_OK;
}

OVL_API int ovl_destroy(ovl_ctx* c) {
    if (!c) return OVL_OK;
    DeviceGuard guard;
    for (Dev* d : c->devs) destroy_dev(d);
    if (c->stage.p) (void)hipHostFree(c->stage.p);
    delete c;
    return OVL_OK;
}

// ----------------------------------------------------------------------------- pinned host memory

OVL_API int ovl_host_alloc(int64_t bytes, void** out_ptr) {
    if (!out_ptr) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "out_ptr is NULL");
    *out_ptr = nullptr;
    if (bytes < 0) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "bytes < 0");
    // fine-grained (coherent): kernels store results into it while host code may hold cached copies of the
    // same lines (a caller reusing its arrays); the coarse-grained kind made no difference in step time
    // (profiles/r02_pack_ab_target.json)
    HIPCHK((ovl_ctx*)nullptr, hipHostMalloc(out_ptr, (size_t)std::max<int64_t>(bytes, 64), kHostShared));
    return OVL_OK;
}

OVL_API int ovl_host_free(void* ptr) {
    if (ptr) HIPCHK((ovl_ctx*)nullptr, hipHostFree(ptr));
    return OVL_OK;
}

OVL_API int ovl_host_register(void* ptr, int64_t bytes) {
    if (!ptr || bytes <= 0) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "NULL pointer or empty range");
    HIPCHK((ovl_ctx*)nullptr, hipHostRegister(ptr, (size_t)bytes, hipHostRegisterPortable));
    return OVL_OK;
}

OVL_API int ovl_host_unregister(void* ptr) {
    if (!ptr) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "NULL pointer");
    HIPCHK((ovl_ctx*)nullptr, hipHostUnregister(ptr));
    return OVL_OK;
}

OVL_API int ovl_host_pool(int32_t* threads, int32_t* sharers, int32_t* cpus, int32_t* packed) {
    CpuShare& cs = CpuShare::get();
    const int n = cs.refresh(true);
    const int t = CopyPool::threads();
    if (threads) *threads = t;
    if (sharers) *sharers = n;
    if (cpus) *cpus = cs.cpus();
    if (packed) *packed = t >= 6 ? 1 : 0;
    return OVL_OK;
}

OVL_API int32_t ovl_host_pool_rule(int32_t cpus, int32_t sharers, int32_t env_threads) {
    return pool_rule(cpus, sharers, env_threads);
}

OVL_API int ovl_set_timing(ovl_ctx* c, int32_t on) {
    if (!c) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    c->timing = on ? 1 : 0;
    return OVL_OK;
}

OVL_API int ovl_last_transfer(const ovl_ctx* c, int64_t* link_bytes, int64_t* packed_pairs) {
    if (!c) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    if (link_bytes) *link_bytes = c->x_link_bytes;
    if (packed_pairs) *packed_pairs = c->x_packed_pairs;
    return OVL_OK;
}

OVL_API int ovl_last_results(const ovl_ctx* c, int64_t* result_bytes, int64_t* record_pairs, int64_t* escapes) {
    if (!c) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    if (result_bytes) *result_bytes = c->x_res_bytes;
    if (record_pairs) *record_pairs = c->x_rec_pairs;
    if (escapes) *escapes = c->x_esc;
    return OVL_OK;
}

OVL_API int ovl_last_pair_list(const ovl_ctx* c, int64_t* in_place_pairs, int64_t* decoded_pairs) {
    if (!c) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    if (in_place_pairs) *in_place_pairs = c->x_ix_pairs;
    if (decoded_pairs) *decoded_pairs = c->x_dec_pairs;
    return OVL_OK;
}

OVL_API int ovl_last_launches(const ovl_ctx* c, int32_t cap, int32_t* device, int32_t* sink, int64_t* pairs,
                              double* ms, int32_t* out_n) {
    if (!c) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    if (cap < 0) return fail(c, OVL_E_ARG, "cap < 0");
    const int32_t n = (int32_t)c->t_launches.size();
    if (out_n) *out_n = n;
    for (int32_t i = 0; i < n && i < cap; ++i) {
        const auto& L = c->t_launches[(size_t)i];
        if (device) device[i] = L.device;
        if (sink) sink[i] = L.sink;
        if (pairs) pairs[i] = L.pairs;
        if (ms) ms[i] = L.ms;
    }
    return OVL_OK;
}

OVL_API int ovl_last_timing(const ovl_ctx* c, double* kernel_ms, double* call_ms) {
    if (!c) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    if (kernel_ms) *kernel_ms = c->t_kernel_ms;
    if (call_ms) *call_ms = c->t_call_ms;
    return OVL_OK;
}
