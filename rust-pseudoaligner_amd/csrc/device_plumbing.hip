// What touches no index: device selection, the synthetic-read device object, and event / allocation / copy plumbing for hosts without their own
// allocator or event API.
#include <hip/hip_runtime.h>

#include "hip_buffer.hpp"
#include "kernels.hpp"
#include "synth_common.hpp"

using namespace pa;

int pa::use_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(PA_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(PA_ERR_INVALID_ARG, "device %d out of range (have %d)", device, n);
    PA_HIP_TRY(hipSetDevice(device));
    return PA_OK;
}

int pa::have_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PA_ERR_NO_DEVICE, "no HIP device available; this library has no CPU fallback");
    return PA_OK;
}

extern "C" {

int pa_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---- synthetic reads on the device ----
struct pa_txome_device {
    int device;
    uint32_t num_tx, read_len;
    uint64_t total;
    DeviceBuffer<uint64_t> d_packed, d_tx_start, d_cum;
};

int pa_txome_upload(const pa_txome* t, uint32_t read_len, int device, pa_txome_device** out) {
    if (!t || !out || read_len == 0 || read_len > PA_MAX_SIM_READ_LEN) return fail(PA_ERR_INVALID_ARG, "bad argument");
    int rc = use_device(device);
    if (rc != PA_OK) return rc;
    std::vector<uint64_t> cum;
    synth::build_cum(t->t.tx_start.data(), t->t.num_tx(), read_len, cum);
    if (cum.back() == 0) return fail(PA_ERR_INVALID_ARG, "no transcript is at least %u bases long", read_len);
    pa_txome_device* d = new pa_txome_device{device, t->t.num_tx(), read_len, cum.back()};
    rc = upload(d->d_packed, t->t.packed);
    if (rc == PA_OK) rc = upload(d->d_tx_start, t->t.tx_start);
    if (rc == PA_OK) rc = upload(d->d_cum, cum);
    if (rc != PA_OK) { pa_txome_device_destroy(d); return rc; }
    *out = d;
    return PA_OK;
}

void pa_txome_device_destroy(pa_txome_device* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    delete t;
}

int pa_simulate_reads_device(const pa_txome_device* t, uint64_t seed, uint32_t sub_rate_ppm, uint64_t first_read, uint64_t n_reads,
                             uint32_t words_per_read, uint64_t* d_tiles, uint32_t* d_lens, void* stream) {
    if (!t || !d_tiles || !d_lens) return fail(PA_ERR_INVALID_ARG, "null argument");
    if (words_per_read < (t->read_len + 31) / 32) return fail(PA_ERR_INVALID_ARG, "words_per_read too small");
    PA_HIP_TRY(hipSetDevice(t->device));
    const int e = launch_simulate(t->d_packed.get(), t->d_tx_start.get(), t->d_cum.get(), t->num_tx, t->total, t->read_len, seed, sub_rate_ppm, first_read,
                                  n_reads, words_per_read, d_tiles, d_lens, static_cast<hipStream_t>(stream));
    if (e) return fail(PA_ERR_HIP, "simulate launch: %s", hipGetErrorString((hipError_t)e));
    return PA_OK;
}

// ---- plumbing for hosts without their own allocator / event API ----
int pa_event_create(void** ev) {
    if (!ev) return fail(PA_ERR_INVALID_ARG, "null argument");
    hipEvent_t e;
    PA_HIP_TRY(hipEventCreate(&e));
    *ev = e;
    return PA_OK;
}
int pa_event_record(void* ev, void* stream) { PA_HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(ev), static_cast<hipStream_t>(stream))); return PA_OK; }
int pa_event_elapsed_ms(void* start, void* stop, float* ms) {
    PA_HIP_TRY(hipEventSynchronize(static_cast<hipEvent_t>(stop)));
    PA_HIP_TRY(hipEventElapsedTime(ms, static_cast<hipEvent_t>(start), static_cast<hipEvent_t>(stop)));
    return PA_OK;
}
int pa_event_destroy(void* ev) { PA_HIP_TRY(hipEventDestroy(static_cast<hipEvent_t>(ev))); return PA_OK; }

int pa_device_malloc(int device, size_t bytes, void** out) {
    if (!out) return fail(PA_ERR_INVALID_ARG, "null argument");
    int rc = use_device(device);
    if (rc != PA_OK) return rc;
    hipError_t e = hipMalloc(out, bytes ? bytes : 16);
    if (e != hipSuccess) return fail(PA_ERR_OOM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return PA_OK;
}
int pa_device_free(void* p) { if (p) PA_HIP_TRY(hipFree(p)); return PA_OK; }
int pa_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) {
    PA_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, static_cast<hipStream_t>(stream)));
    return PA_OK;
}
int pa_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) {
    PA_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    PA_HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return PA_OK;
}
int pa_memset_device(void* dst, int value, size_t bytes, void* stream) {
    PA_HIP_TRY(hipMemsetAsync(dst, value, bytes, static_cast<hipStream_t>(stream)));
    return PA_OK;
}
int pa_stream_synchronize(void* stream) { PA_HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream))); return PA_OK; }

}  // extern "C"
