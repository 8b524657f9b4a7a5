// g++ -std=c++17 -O1 -fsanitize=thread -pthread -I point_sam_amd/csrc tests/host/knob_threads.cpp -o knob_threads && ./knob_threads
// Race check of csrc/knob.h on the CPU (not a pytest test, needs no GPU): eight threads, half of them forcing two knobs to alternating values, half of them
// reading both.  ThreadSanitizer must stay silent, and every value read must be one of the values written, the environment's, or the default.
#include "knob.h"

#include <cstdio>
#include <thread>
#include <vector>

static psam_knob k_env("KNOB_THREADS_ENV", 7);      // has an environment name (run with KNOB_THREADS_ENV=5 to exercise that path)
static psam_knob k_plain(nullptr, 3);               // only a hook sets it

int main() {
    constexpr int ITER = 200000, WRITERS = 4, READERS = 4;
    const char* e = std::getenv("KNOB_THREADS_ENV");
    const int env_value = e ? std::atoi(e) : 7;
    std::atomic<long> bad{0};
    std::vector<std::thread> threads;
    for (int t = 0; t < WRITERS; ++t)
        threads.emplace_back([t] {
            for (int i = 0; i < ITER; ++i) {
                const int v = (i & 1) ? -1 : (t & 1);      // -1 hands the knob back, 0 / 1 force it
                k_env.force(v);
                k_plain.force(v);
            }
        });
    for (int t = 0; t < READERS; ++t)
        threads.emplace_back([&bad, env_value] {
            for (int i = 0; i < ITER; ++i) {
                const int ge = k_env.get(), fe = k_env.forced(), gp = k_plain.get(), fp = k_plain.forced();
                const bool ok = (ge == 0 || ge == 1 || ge == env_value) && (fe >= -1 && fe <= 1) && (gp == 0 || gp == 1 || gp == 3) && (fp >= -1 && fp <= 1);
                if (!ok) bad.fetch_add(1);
            }
        });
    for (std::thread& th : threads) th.join();
    k_env.force(-1);
    k_plain.force(-1);
    const bool ok = bad.load() == 0 && k_env.get() == env_value && k_plain.get() == 3 && k_env.forced() == -1;
    std::printf("knob_threads: %ld unexpected values, %s\n", bad.load(), ok ? "OK" : "FAILED");
    return ok ? 0 : 1;
}
