// The failure path of abi_internal.h's launch(), on a machine WITHOUT a device: a refused launch answers RL_ERR_HIP and a
// message that names the kernel and carries HIP's reason.  With a device present nothing is launched: the program says
// that it skipped (tests/test_launch_host.py compiles and runs it).
#include "../pyracecarsimulator_amd/csrc/abi_internal.h"

static char g_msg[512];
int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return code;
}

struct ProbeParams {
    int rows, cols;
    float res;
};
__global__ void launch_probe_kernel(ProbeParams, const double *, double *, size_t) {}

#define REQUIRE(cond)                                                  \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("FAILED %s (code %d, message '%s')\n", #cond, rc, g_msg); \
            return 1;                                                  \
        }                                                              \
    } while (0)

int main()
{
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0) {
        printf("skipped: %d device(s) present, nothing launched\n", n_dev);
        return 0;
    }
    (void)hipGetLastError();                    // (the count's own error is not the launch's)
    const DevPtr<double> in;                    // (owns nothing: reads as a null const double *)
    const int count = 7;
    const int rc = launch("launch_probe_kernel", launch_probe_kernel, dim3(1), dim3(64), 0, nullptr, ProbeParams{4, 4, 0.5f}, in,
                          nullptr, count);
    const char *head = "launch_probe_kernel launch failed: ";
    REQUIRE(rc == RL_ERR_HIP);
    REQUIRE(strncmp(g_msg, head, strlen(head)) == 0);
    const char *reason = g_msg + strlen(head);
    REQUIRE(*reason != '\0' && strcmp(reason, hipGetErrorString(hipSuccess)) != 0);
    // HIP's reason is one of its own strings: the one of the error the runtime keeps answering without a device
    const hipError_t again = hipSetDevice(0);
    REQUIRE(again != hipSuccess);
    printf("refused: code %d, '%s' (hipSetDevice: '%s')\n", rc, g_msg, hipGetErrorString(again));
    return 0;
}
