// switches_selftest.cpp -- every accessor of flux_amd/csrc/flux_switches.h over unset, "", "0", "1", "-3", "abc", "7x" and its own edge
// values, set and read in turn in one process (nothing may be cached).  Prints `<variable> <unset | [value]> <result>`, one line a
// read; tests/test_switches.py holds the expected column.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../flux_amd/csrc/flux_switches.h"

template <class F>
static void rows(const char *name, std::initializer_list<const char *> more, F print_result) {
    auto row = [&](const char *v) {
        if (v) setenv(name, v, 1);
        else unsetenv(name);
        if (v) std::printf("%s [%s] ", name, v);
        else std::printf("%s unset ", name);
        print_result();
        std::printf("\n");
    };
    for (const char *v : {(const char *)nullptr, "", "0", "1", "-3", "abc", "7x"}) row(v);
    for (const char *v : more) row(v);
    unsetenv(name);
}

int main() {
    using namespace flux;
    for (const char *name :
         {kEnvSampleTables, kEnvThroughputTable, kEnvLobeFrames, kEnvPlaneAxis, kEnvSampleOrder, kEnvSplitDepthCut, kEnvSplitUniformA})
        rows(name, {}, [&] { std::printf("%d", switch_off(name) ? 1 : 0); });
    rows("FLUX_SPLIT_HITQ_CAP", {"67", "-5", "110", "200"}, [] { std::printf("%u", hitq_cap(110u)); });
    rows("FLUX_SPLIT_HITQ_TAKE_AT", {"64", "100"}, [] { std::printf("%u", hitq_take_at(46u)); });
    rows("FLUX_DENOISE_LDS_LEVELS", {"8"}, [] { std::printf("%d", denoise_lds_levels(3)); });
    rows("FLUX_BUILD_THREADS", {"16", "99"}, [] { std::printf("%u", build_threads()); });
    rows("FLUX_RCCL_LIB", {"/opt/lib/librccl.so"}, [] { const char *p = rccl_lib(); std::printf("%s", p ? p : "(null)"); });
    std::printf("all ok\n");
    return 0;
}
