// test_dev_buf.cpp -- DevBuf (slam-tricks_amd/csrc/common.hpp), the one owner of device memory, and loss_table_check
// (robust_loss.hpp), the host check both set_loss entry points share.  No HIP runtime is linked: hipMalloc / hipFree /
// hipGetErrorString are defined HERE over malloc / free, with a table of the live addresses and a switch that makes the next
// hipMalloc fail.  After every step the library's live count must equal the table's size; a double free or a free of an unknown
// address aborts the run.  Prints "dev_buf ok" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../slam-tricks_amd/csrc/robust_loss.hpp"

namespace stba { thread_local std::string g_last_error; }
using namespace stba;

static std::set<void*> g_table;
static size_t g_last_bytes = 0;
static int g_mallocs = 0, g_frees = 0;
static bool g_fail_next = false;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

extern "C" hipError_t hipMalloc(void** p, size_t bytes) {
    if (g_fail_next) { g_fail_next = false; *p = reinterpret_cast<void*>(0x1); return hipErrorOutOfMemory; }    // (a failed call may leave garbage)
    *p = std::malloc(bytes);
    g_table.insert(*p);
    g_last_bytes = bytes;
    ++g_mallocs;
    return hipSuccess;
}
extern "C" hipError_t hipFree(void* p) {
    if (!p) return hipSuccess;
    CHECK(g_table.erase(p) == 1);          // never an address that is not live: no double free, no stray free
    std::free(p);
    ++g_frees;
    return hipSuccess;
}
extern "C" const char* hipGetErrorString(hipError_t) { return "out of memory (test)"; }

static long long live() { return g_live_device_buffers.load(); }
#define IN_STEP() CHECK(live() == (long long)g_table.size())

struct Several { DevBuf<double> a, b; DevBuf<int> c, d; };

static void test_dev_buf() {
    IN_STEP();
    CHECK(live() == 0);
    {   // alloc, then the destructor frees once
        DevBuf<double> x;
        CHECK(!x && x.get() == nullptr);
        CHECK(x.alloc(10) == STBA_OK);
        CHECK(x && g_last_bytes == 10 * sizeof(double) && g_table.count(x.get()) == 1);
        double* raw = x;                    // the implicit conversion
        CHECK(raw == x.get() && x + 3 == raw + 3);
        IN_STEP();
        CHECK(live() == 1);
    }
    IN_STEP();
    CHECK(live() == 0 && g_mallocs == 1 && g_frees == 1);
    {   // alloc(0) yields one element
        DevBuf<int> z;
        CHECK(z.alloc(0) == STBA_OK && z && g_last_bytes == sizeof(int));
        IN_STEP();
        // alloc on a buffer that holds something frees that first
        const int frees = g_frees;
        CHECK(z.alloc(4) == STBA_OK && g_frees == frees + 1 && live() == 1);
        IN_STEP();
    }
    IN_STEP();
    {   // move construction transfers
        DevBuf<double> a;
        CHECK(a.alloc(3) == STBA_OK);
        double* pa = a;
        DevBuf<double> b(std::move(a));
        CHECK(!a && b.get() == pa && live() == 1);
        IN_STEP();
        // move assignment frees what the target held
        DevBuf<double> c;
        CHECK(c.alloc(5) == STBA_OK);
        double* pc = c;
        IN_STEP();
        c = std::move(b);
        CHECK(!b && c.get() == pa && g_table.count(pc) == 0 && g_table.count(pa) == 1 && live() == 1);
        IN_STEP();
        // assignment of an empty buffer releases
        c = DevBuf<double>();
        CHECK(!c && live() == 0);
        IN_STEP();
        // self-move is harmless
        CHECK(c.alloc(2) == STBA_OK);
        double* ps = c;
        DevBuf<double>& same = c;
        c = std::move(same);
        CHECK(c.get() == ps && live() == 1);
        IN_STEP();
        // reset twice is harmless
        c.reset();
        CHECK(!c && live() == 0);
        c.reset();
        CHECK(!c && live() == 0);
        IN_STEP();
    }
    IN_STEP();
    {   // a failed alloc: empty buffer, STBA_ERR_ALLOC with dev_alloc's message, the count unchanged
        DevBuf<double> f;
        const long long before = live();
        g_fail_next = true;
        CHECK(f.alloc(8) == STBA_ERR_ALLOC);
        CHECK(!f && f.get() == nullptr && live() == before);
        CHECK(g_last_error == "hipMalloc: out of memory (test)");
        IN_STEP();
        // ... and what the buffer held before the failed call is gone, not leaked
        CHECK(f.alloc(8) == STBA_OK);
        g_fail_next = true;
        CHECK(f.alloc(8) == STBA_ERR_ALLOC && !f && live() == before);
        IN_STEP();
    }
    IN_STEP();
    {   // a struct of several, destroyed after a partial failure, frees exactly what was allocated
        const int m0 = g_mallocs, f0 = g_frees;
        {
            Several s;
            CHECK(s.a.alloc(4) == STBA_OK && s.b.alloc(4) == STBA_OK);
            g_fail_next = true;
            CHECK(s.c.alloc(4) == STBA_ERR_ALLOC);
            CHECK(live() == 2 && !s.c && !s.d);
            IN_STEP();
        }
        CHECK(g_mallocs - m0 == 2 && g_frees - f0 == 2 && live() == 0);
        IN_STEP();
    }
    {   // an array member, as the engines' cams[2]
        DevBuf<double> pair[2];
        CHECK(pair[0].alloc(7) == STBA_OK && pair[1].alloc(7) == STBA_OK && live() == 2);
        std::swap(pair[0], pair[1]);
        CHECK(live() == 2);
        IN_STEP();
    }
    IN_STEP();
    CHECK(live() == 0 && g_table.empty() && g_mallocs == g_frees);
}

static void expect_refused(const char* noun, const std::vector<int>& kind, const double* a, const double* b, const double* scale,
                           const std::string& message) {
    std::vector<double> ha, hb, hs;
    g_last_error.clear();
    CHECK(loss_table_check("who", noun, kind.size(), kind.data(), a, b, scale, ha, hb, hs) == STBA_ERR_INVALID_ARGUMENT);
    if (g_last_error != message) std::printf("got:  %s\nwant: %s\n", g_last_error.c_str(), message.c_str());
    CHECK(g_last_error == message);
}

static void test_loss_table() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> ha, hb, hs;
    {   // a good table: the defaults where a kind does not read a parameter, the caller's values elsewhere
        const std::vector<int> kind = {STBA_LOSS_TRIVIAL, STBA_LOSS_HUBER, STBA_LOSS_TOLERANT, STBA_LOSS_TUKEY};
        const double a[4] = {-5.0, 2.0, 3.0, 4.0}, b[4] = {nan, -1.0, 0.5, 0.0}, scale[4] = {0.0, 1.5, 2.5, 3.5};
        CHECK(loss_table_check("who", "observation", 4, kind.data(), a, b, scale, ha, hb, hs) == STBA_OK);
        CHECK((ha == std::vector<double>{1.0, 2.0, 3.0, 4.0}));
        CHECK((hb == std::vector<double>{1.0, 1.0, 0.5, 1.0}));
        CHECK((hs == std::vector<double>{0.0, 1.5, 2.5, 3.5}));
        // no scale, no b, all TRIVIAL without a: every default
        const std::vector<int> triv = {STBA_LOSS_TRIVIAL, STBA_LOSS_TRIVIAL};
        CHECK(loss_table_check("who", "edge", 2, triv.data(), nullptr, nullptr, nullptr, ha, hb, hs) == STBA_OK);
        CHECK((ha == std::vector<double>{1.0, 1.0}) && hb == ha && hs == ha);
        CHECK(loss_table_check("who", "edge", 0, triv.data(), nullptr, nullptr, nullptr, ha, hb, hs) == STBA_OK && ha.empty());
    }
    const double a2[2] = {1.0, 1.0};
    expect_refused("observation", {STBA_LOSS_HUBER, 7}, a2, nullptr, nullptr, "who: observation 1: unknown loss kind 7");
    expect_refused("edge", {-1, STBA_LOSS_HUBER}, a2, nullptr, nullptr, "who: edge 0: unknown loss kind -1");
    expect_refused("observation", {STBA_LOSS_TRIVIAL, STBA_LOSS_CAUCHY}, nullptr, nullptr, nullptr,
                   "who: observation 1: the loss parameter a must be finite and positive");
    const double a_zero[2] = {1.0, 0.0}, a_neg[2] = {-2.0, 1.0}, a_inf[2] = {1.0, inf}, a_nan[2] = {nan, 1.0};
    expect_refused("edge", {STBA_LOSS_HUBER, STBA_LOSS_HUBER}, a_zero, nullptr, nullptr, "who: edge 1: the loss parameter a must be finite and positive");
    expect_refused("edge", {STBA_LOSS_HUBER, STBA_LOSS_HUBER}, a_neg, nullptr, nullptr, "who: edge 0: the loss parameter a must be finite and positive");
    expect_refused("observation", {STBA_LOSS_ARCTAN, STBA_LOSS_SOFTLONE}, a_inf, nullptr, nullptr,
                   "who: observation 1: the loss parameter a must be finite and positive");
    expect_refused("observation", {STBA_LOSS_TUKEY, STBA_LOSS_TUKEY}, a_nan, nullptr, nullptr,
                   "who: observation 0: the loss parameter a must be finite and positive");
    expect_refused("observation", {STBA_LOSS_HUBER, STBA_LOSS_TOLERANT}, a2, nullptr, nullptr,
                   "who: observation 1: the loss parameter b must be finite and positive");
    const double b_bad[2] = {1.0, -1.0};
    expect_refused("edge", {STBA_LOSS_HUBER, STBA_LOSS_TOLERANT}, a2, b_bad, nullptr, "who: edge 1: the loss parameter b must be finite and positive");
    const double s_neg[2] = {1.0, -0.5}, s_nan[2] = {nan, 1.0};
    expect_refused("observation", {STBA_LOSS_TRIVIAL, STBA_LOSS_TRIVIAL}, nullptr, nullptr, s_neg,
                   "who: observation 1: the loss scale must be finite and not negative");
    expect_refused("edge", {STBA_LOSS_HUBER, STBA_LOSS_HUBER}, a2, nullptr, s_nan, "who: edge 0: the loss scale must be finite and not negative");
}

int main() {
    test_dev_buf();
    test_loss_table();
    std::printf("dev_buf ok\n");
    return 0;
}
