// grow_buf.h on the host (no GPU, no HIP): GrowBuf and the staged pair's
// reserve over a malloc-backed memory kind that counts its calls, logs their
// order and can fail the next allocation.  Built with ASan + UBSan, leak check
// on, and run as its own process by tests/test_grow_buf_native.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../photohive_dsp_amd/csrc/grow_buf.h"

namespace {

int g_fail = 0;
#define CHECK(x)                                              \
    do {                                                      \
        if (!(x)) {                                           \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); \
            g_fail++;                                         \
        }                                                     \
    } while (0)

// One kind per tag, so a pair's two blocks count apart.
template <int Tag>
struct TestMem {
    static int allocs, frees, idles;
    static bool fail_next;
    static size_t last_size;
    static std::string log, message;          // 'i' idle, 'f' free, 'a' alloc, 'x' failed alloc
    static std::set<void*> live;
    static void* alloc(size_t sz) {
        if (fail_next) {
            fail_next = false;
            log += 'x';
            return nullptr;
        }
        void* p = malloc(sz);
        memset(p, 0xA5, sz);                  // the whole block is the caller's
        allocs++;
        last_size = sz;
        live.insert(p);
        log += 'a';
        return p;
    }
    static void free(void* p) {
        CHECK(live.erase(p) == 1);            // a live block, freed once
        ::free(p);
        frees++;
        log += 'f';
    }
    static void idle() {
        idles++;
        log += 'i';
    }
    static void failed(size_t sz) { message = "alloc of " + std::to_string(sz) + " bytes failed"; }
    static void reset() {
        CHECK(live.empty());
        allocs = frees = idles = 0;
        fail_next = false;
        last_size = 0;
        log.clear();
        message.clear();
    }
};
template <int T> int TestMem<T>::allocs = 0;
template <int T> int TestMem<T>::frees = 0;
template <int T> int TestMem<T>::idles = 0;
template <int T> bool TestMem<T>::fail_next = false;
template <int T> size_t TestMem<T>::last_size = 0;
template <int T> std::string TestMem<T>::log;
template <int T> std::string TestMem<T>::message;
template <int T> std::set<void*> TestMem<T>::live;

using M = TestMem<0>;
using Buf = phd::GrowBuf<M>;
size_t grown(size_t need) { return need + need / 4 + 4096; }

void test_keep_and_grow() {
    M::reset();
    Buf b;
    CHECK(b.as() == nullptr && b.capacity() == 0);
    CHECK(b.ensure(1000) && M::log == "a");   // an empty buffer: no idle, no free
    CHECK(b.capacity() == grown(1000) && M::last_size == grown(1000));
    void* p = b.as();
    CHECK(p && M::live.count(p));
    memset(b.as<char>(), 1, b.capacity());
    // need <= capacity: the same pointer, no call at all
    for (size_t need : {size_t(0), size_t(1), size_t(1000), grown(1000)}) {
        CHECK(b.ensure(need) && b.as() == p && b.capacity() == grown(1000));
    }
    CHECK(M::log == "a");
    // one byte more: exactly idle, free, alloc of need + need / 4 + 4096, in that order
    const size_t need = grown(1000) + 1;
    CHECK(b.ensure(need) && M::log == "aifa");
    CHECK(M::idles == 1 && M::frees == 1 && M::allocs == 2);
    CHECK(b.capacity() == grown(need) && M::last_size == grown(need) && M::live.size() == 1);
    memset(b.as<char>(), 2, b.capacity());
    b.release();
    CHECK(M::log == "aifaf" && M::live.empty());
}

void test_failure() {
    M::reset();
    Buf b;
    // a failed first allocation
    M::fail_next = true;
    CHECK(!b.ensure(64) && b.as() == nullptr && b.capacity() == 0);
    CHECK(M::message == "alloc of " + std::to_string(grown(64)) + " bytes failed" && M::log == "x");
    M::message.clear();
    CHECK(b.ensure(64) && b.as() && b.capacity() == grown(64) && M::log == "xa" && M::message.empty());
    // a failed growth: the old block is gone (idle, free), {nullptr, 0}, then a fresh allocation
    M::fail_next = true;
    const size_t big = 100000;
    CHECK(!b.ensure(big) && b.as() == nullptr && b.capacity() == 0 && M::log == "xaifx");
    CHECK(M::message == "alloc of " + std::to_string(grown(big)) + " bytes failed" && M::live.empty());
    CHECK(b.ensure(1) && b.capacity() == grown(1) && M::log == "xaifxa");   // (nothing to wait for or free)
    CHECK(b.ensure(big) && b.capacity() == grown(big) && M::log == "xaifxaifa");
    b.as<char>()[big - 1] = 3;
    b.release();
    CHECK(M::allocs == M::frees && M::allocs == 3 && M::idles == 2);
}

void test_release() {
    M::reset();
    Buf b;
    b.release();                              // empty: nothing to free
    CHECK(M::log.empty());
    CHECK(b.ensure(10));
    b.release();
    CHECK(b.as() == nullptr && b.capacity() == 0 && M::log == "af");
    b.release();                              // twice
    CHECK(b.as() == nullptr && b.capacity() == 0 && M::log == "af");
    CHECK(b.ensure(5) && b.as() && b.capacity() == grown(5) && M::log == "afa");   // release, then ensure: afresh
    b.as<char>()[grown(5) - 1] = 4;
    b.release();
    CHECK(M::log == "afaf");
}

void test_zero() {
    M::reset();
    Buf b;
    CHECK(b.ensure(0) && b.as() != nullptr && b.capacity() == 4096 && M::log == "a");
    CHECK(b.ensure(0) && M::log == "a");
    b.release();
}

void test_staged() {
    using D = TestMem<1>;
    using P = TestMem<2>;
    D::reset();
    P::reset();
    phd::StagedBuf<D, P> s;
    CHECK(s.reserve(3072, 512) && D::log == "a" && P::log == "a");
    CHECK(s.d.capacity() == grown(3072) && s.h.capacity() == grown(512));
    void* d0 = s.d.as();
    void* h0 = s.h.as();
    CHECK(s.reserve(grown(3072), 100) && s.d.as() == d0 && s.h.as() == h0);        // both kept
    CHECK(s.reserve(20000, 100) && s.d.as() && s.h.as() == h0 && D::log == "aifa" && P::log == "a");   // one grows
    CHECK(s.reserve(20000, 9000) && D::log == "aifa" && P::log == "aifa");
    // a failed device block: false, the pinned block untouched; then both afresh
    D::fail_next = true;
    CHECK(!s.reserve(100000, 100000) && s.d.as() == nullptr && s.d.capacity() == 0 && P::log == "aifa");
    CHECK(!D::message.empty() && P::message.empty());
    P::fail_next = true;
    CHECK(!s.reserve(100000, 100000) && s.d.capacity() == grown(100000) && s.h.as() == nullptr);
    CHECK(P::message == "alloc of " + std::to_string(grown(100000)) + " bytes failed");
    CHECK(s.reserve(100000, 100000) && s.h.capacity() == grown(100000));
    memset(s.d.as<char>(), 5, s.d.capacity());
    memset(s.h.as<char>(), 6, s.h.capacity());
    s.release();
    s.release();
    CHECK(D::live.empty() && P::live.empty() && D::allocs == D::frees && P::allocs == P::frees);
}

}  // namespace

int main() {
    test_keep_and_grow();
    test_failure();
    test_release();
    test_zero();
    test_staged();
    CHECK(M::live.empty() && TestMem<1>::live.empty() && TestMem<2>::live.empty());
    if (g_fail) return printf("grow_buf: %d FAILED\n", g_fail), 1;
    printf("grow_buf OK\n");
    return 0;
}
