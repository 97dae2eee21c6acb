// Library-wide entry points of the C ABI (include/peahip.h): version, thread-local error text, device probe.
#include <cstring>
#include <map>
#include <mutex>
#include <utility>

#include "common.h"

namespace pea {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

const char *get_error() { return g_err; }

int device_cu_count(int *n_cu) {
    static int cached = 0;
    if (!cached) {
        hipDeviceProp_t prop;
        int dev = 0;
        PEA_HIP(hipGetDevice(&dev));
        PEA_HIP(hipGetDeviceProperties(&prop, dev));
        cached = prop.multiProcessorCount;
    }
    *n_cu = cached;
    return PEA_OK;
}

// The one place the library raises a kernel's dynamic-LDS limit.  The HIP attribute belongs to the kernel on one device,
// so what has been asked for is remembered per (device, kernel).
int ensure_dynamic_lds(const void *kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return PEA_OK;
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> raised;
    int dev = 0;
    PEA_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    size_t &have = raised[{dev, kernel}];
    if (bytes <= have) return PEA_OK;
    PEA_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    have = bytes;
    return PEA_OK;
}

}  // namespace pea

extern "C" const char *pea_version(void) { return "peahip 0.1.0 (gfx950)"; }

extern "C" const char *pea_last_error(void) { return pea::get_error(); }

extern "C" int pea_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    int ok = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, i) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    return ok;
}
