// The milliseconds between the N phases of one call, on the null stream (pa_bus_correct_phase_ms, pa_bus_knee_phase_ms). Included by .hip
// sources only.
#pragma once
#include <hip/hip_runtime.h>

#include "hip_buffer.hpp"

namespace pa {

template <int N>
struct PhaseClock {
    hipEvent_t ev[N + 1] = {};
    int made = 0;
    ~PhaseClock() { for (int i = 0; i < made; ++i) (void)hipEventDestroy(ev[i]); }
    int open() {
        for (; made <= N; ++made) PA_HIP_TRY(hipEventCreate(&ev[made]));
        return PA_OK;
    }
    int mark(int i) { PA_HIP_TRY(hipEventRecord(ev[i], nullptr)); return PA_OK; }
    // ev[0 .. marked] were recorded: ms[i] = the time from ev[i] to ev[i + 1], 0 for a phase that was not marked. Synchronises
    int close(float (&ms)[N], int marked = N) {
        PA_HIP_TRY(hipEventSynchronize(ev[marked]));
        for (int i = 0; i < N; ++i) {
            ms[i] = 0.0f;
            if (i < marked) PA_HIP_TRY(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
        }
        return PA_OK;
    }
};

}  // namespace pa
