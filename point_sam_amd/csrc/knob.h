// The one mechanism behind every behaviour switch of the library (the table of all of them: INTEGRATION.md, "Switches").  A switch has an optional
// environment variable, a default, and a value a psam_*_force_* / psam_*_set_* hook may force:
//     static psam_knob k_knn_band("PSAM_KNN_BAND", 1);
//     PSAM_API void psam_knn_force_band(int32_t mode) { k_knn_band.force(mode); }
//     ... k_knn_band.get() ...
// Host only and plain C++17 (no HIP header): a CPU program can include this file on its own (tests/host/knob_threads.cpp).
// The environment is read ONCE per process, lazily by the first get() that needs it, and parsed with atoi.  Every member is a relaxed atomic access, so
// any number of threads may call get(), forced() and force() at the same time; a get() that races a force() returns the value before or after it.
// getenv appears in the library's sources in this file only.
#pragma once
#include <atomic>
#include <climits>
#include <cstdlib>

class psam_knob {
public:
    constexpr psam_knob(const char* env, int dflt) : env_(env), dflt_(dflt) {}      // env: the variable's name, or nullptr for a switch only a hook sets
    // the forced value if one >= 0 is set, else the environment's, else the default
    int get() const {
        const int f = forced();
        return f >= 0 ? f : from_env();
    }
    // get() for a switch that counts something: an environment value <= 0 means the default
    int get_positive() const {
        const int v = get();
        return v > 0 ? v : dflt_;
    }
    // the hook's raw value (-1: none): tells "forced on" from "on by default or by the environment"
    int forced() const { return forced_.load(std::memory_order_relaxed); }
    void force(int v) { forced_.store(v, std::memory_order_relaxed); }

private:
    int from_env() const {
        long long c = cached_.load(std::memory_order_relaxed);
        if (c == UNREAD) {      // threads that arrive together all read the same environment and store the same value
            const char* e = env_ ? std::getenv(env_) : nullptr;
            c = e ? std::atoi(e) : dflt_;
            cached_.store(c, std::memory_order_relaxed);
        }
        return (int)c;
    }
    static constexpr long long UNREAD = LLONG_MIN;      // no int
    const char* env_;
    int dflt_;
    std::atomic<int> forced_{-1};
    mutable std::atomic<long long> cached_{UNREAD};
};

// The two real-valued tuning constants: the environment's value (atof), dflt when it is unset.  Read once per process and thread-safely as the initialiser
// of a function-local static: `static const double x = psam_env_double("NAME", dflt);`.
static inline double psam_env_double(const char* name, double dflt) {
    const char* e = std::getenv(name);
    return e ? std::atof(e) : dflt;
}
