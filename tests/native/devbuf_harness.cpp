// Host harness for retargetvid_amd/csrc/svc_devbuf.h: DevBuf's ownership rule over counting stubs of the HIP allocator.
// A stand-alone program (tests/test_devbuf_host.py builds it with -fsanitize=address,undefined and runs it); it links without
// the HIP runtime: hipMalloc, hipFree, hipGetErrorString and svc_set_error are defined here.  Exit status 0 only if every check
// held and no block is live at the end.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <set>
#include <tuple>
#include <type_traits>
#include <utility>

#include "../../retargetvid_amd/csrc/svc_devbuf.h"

static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "DevBuf copies");
static_assert(!std::is_copy_constructible<ResampleTab>::value && !std::is_copy_assignable<ResampleTab>::value, "ResampleTab copies");
static_assert(std::is_nothrow_move_constructible<DevBuf>::value && std::is_nothrow_move_assignable<DevBuf>::value, "DevBuf moves");
static_assert(!std::is_copy_constructible<std::pair<DevBuf, DevBuf>>::value, "a pair of DevBuf copies");

// ---- the stubs
static std::set<void *> g_live;             // blocks handed out and not yet freed
static int g_mallocs = 0, g_frees = 0, g_bad_frees = 0;
static int g_fail_at = 0;                   // the knob: the g_fail_at-th allocation from now fails (0: none)
static char g_error[256];

extern "C" hipError_t hipMalloc(void **ptr, size_t size) {
    if (g_fail_at && --g_fail_at == 0) return hipErrorOutOfMemory;      // (*ptr is left alone, as the runtime leaves it)
    *ptr = malloc(size);
    g_live.insert(*ptr);
    ++g_mallocs;
    return hipSuccess;
}
extern "C" hipError_t hipFree(void *ptr) {
    if (!g_live.erase(ptr)) { ++g_bad_frees; return hipErrorInvalidValue; }    // never handed out, or freed twice
    free(ptr);
    ++g_frees;
    return hipSuccess;
}
extern "C" const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
void svc_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++g_failures; fprintf(stderr, "devbuf_harness:%d: %s\n", __LINE__, #cond); } } while (0)
static bool live(const void *p) { return g_live.count(const_cast<void *>(p)) != 0; }

// ---- the shapes of the library's own call sites
// cv_tab (svc_frames.hip): a local buffer, an upload that may fail, then the store into the handle's map
static int like_cv_tab(std::map<int, DevBuf> &tabs, int key, bool upload_fails, const void **out) {
    auto it = tabs.find(key);
    if (it == tabs.end()) {
        DevBuf buf;
        int rc = buf.ensure(40);
        if (rc) return rc;
        if (upload_fails) return SVC_E_HIP;                 // the early return between ensure and the store
        it = tabs.emplace(key, std::move(buf)).first;
    }
    *out = it->second.p;
    return SVC_OK;
}
// ensure_shrink_tables (svc_tail.hip): a pair of tables, the second of which may fail
static int like_shrink_tables(std::map<int, std::pair<DevBuf, DevBuf>> &tabs, int key) {
    std::pair<DevBuf, DevBuf> t;
    int rc;
    if ((rc = t.first.ensure(24))) return rc;
    if ((rc = t.second.ensure(48))) return rc;
    tabs.emplace(key, std::move(t));
    return SVC_OK;
}
// lz_upload (svc_frames.hip): the coefficients go to a local first and are moved into the table last
static int like_lz_upload(ResampleTab &t, bool upload_fails) {
    if (t.coeff.p) return SVC_OK;
    int rc = t.bounds.ensure(16);
    if (rc) return rc;
    DevBuf c;
    if ((rc = c.ensure(56))) return rc;
    if (upload_fails) return SVC_E_HIP;
    t.coeff = std::move(c);
    return SVC_OK;
}

int main() {
    {   // ensure: a no-op when large enough, else the old block is freed exactly once, then a new one made
        DevBuf b;
        CHECK(b.p == nullptr && b.bytes == 0);
        CHECK(b.ensure(16) == SVC_OK && b.bytes == 16 && g_mallocs == 1 && g_frees == 0);
        void *first = b.p;
        CHECK(b.ensure(8) == SVC_OK && b.p == first && b.bytes == 16 && g_mallocs == 1 && g_frees == 0);
        CHECK(b.ensure(64) == SVC_OK && b.bytes == 64 && g_mallocs == 2 && g_frees == 1 && !live(first) && live(b.p));
        // a failed growth has freed the old block already and leaves the buffer empty, with the library's message
        void *second = b.p;
        g_fail_at = 1;
        CHECK(b.ensure(128) == SVC_E_NOMEM && b.p == nullptr && b.bytes == 0 && g_frees == 2 && !live(second));
        CHECK(!strcmp(g_error, "hipMalloc(128) failed: out of memory"));
        CHECK(b.ensure(32) == SVC_OK && g_mallocs == 3);
        b.release();
        CHECK(b.p == nullptr && b.bytes == 0 && g_frees == 3);
        b.release();                                        // a second release is a no-op
        CHECK(g_frees == 3);
        CHECK(b.ensure(32) == SVC_OK);
    }
    CHECK(g_mallocs == 4 && g_frees == 4 && g_live.empty());            // the destructor freed the last block

    {   // move construction, move assignment, self-move
        DevBuf a;
        CHECK(a.ensure(32) == SVC_OK);
        void *pa = a.p;
        const int frees = g_frees;
        DevBuf b(std::move(a));
        CHECK(a.p == nullptr && a.bytes == 0 && b.p == pa && b.bytes == 32 && g_frees == frees && live(pa));
        DevBuf c;
        CHECK(c.ensure(8) == SVC_OK);
        void *pc = c.p;
        c = std::move(b);                                   // the target's old block goes first
        CHECK(b.p == nullptr && b.bytes == 0 && c.p == pa && c.bytes == 32 && g_frees == frees + 1 && !live(pc) && live(pa));
        DevBuf &self = c;
        c = std::move(self);
        CHECK(c.p == pa && c.bytes == 32 && g_frees == frees + 1 && live(pa));
        b = std::move(a);                                   // empty into empty
        CHECK(b.p == nullptr && g_frees == frees + 1);
    }
    CHECK(g_mallocs == g_frees && g_bad_frees == 0 && g_live.empty());

    {   // a moved buffer in a map (ensure_ring_delta reads the pointer from the entry), then the map goes
        std::map<int, DevBuf> m;
        DevBuf buf;
        CHECK(buf.ensure(100) == SVC_OK);
        void *p = buf.p;
        const void *entry = m.emplace(7, std::move(buf)).first->second.p;
        CHECK(entry == p && buf.p == nullptr && live(p));
        const int frees = g_frees;
        m.clear();
        CHECK(g_frees == frees + 1 && !live(p));
    }
    CHECK(g_mallocs == g_frees && g_bad_frees == 0 && g_live.empty());

    {   // cv_tab: the early return frees the local; the next call builds the table, and later calls find it
        std::map<int, DevBuf> tabs;
        const void *out = nullptr, *again = nullptr;
        const int mallocs = g_mallocs;
        CHECK(like_cv_tab(tabs, 1, true, &out) == SVC_E_HIP && tabs.empty() && g_live.empty() && g_mallocs == mallocs + 1);
        g_fail_at = 1;
        CHECK(like_cv_tab(tabs, 1, false, &out) == SVC_E_NOMEM && tabs.empty() && g_live.empty());
        CHECK(like_cv_tab(tabs, 1, false, &out) == SVC_OK && out && live(out) && g_live.size() == 1);
        CHECK(like_cv_tab(tabs, 1, false, &again) == SVC_OK && again == out && g_live.size() == 1);
    }
    CHECK(g_mallocs == g_frees && g_bad_frees == 0 && g_live.empty());

    {   // ensure_shrink_tables: the second table fails, and the first is not lost
        std::map<int, std::pair<DevBuf, DevBuf>> tabs;
        g_fail_at = 2;
        CHECK(like_shrink_tables(tabs, 3) == SVC_E_NOMEM && tabs.empty() && g_live.empty());
        CHECK(like_shrink_tables(tabs, 3) == SVC_OK && tabs.size() == 1 && g_live.size() == 2);
        CHECK(live(tabs.find(3)->second.first.p) && live(tabs.find(3)->second.second.p));
    }
    CHECK(g_mallocs == g_frees && g_bad_frees == 0 && g_live.empty());

    {   // lz_tab / lz_upload: a ResampleTab moves into its map, is uploaded in place, and survives a failed upload
        std::map<std::pair<int, int>, ResampleTab> tabs;
        ResampleTab t;
        t.ksize = 3;
        t.coeff_host.assign(12, 1);
        ResampleTab &e = tabs.emplace(std::make_pair(4, 2), std::move(t)).first->second;
        CHECK(e.ksize == 3 && e.coeff_host.size() == 12 && !e.coeff.p);
        CHECK(like_lz_upload(e, true) == SVC_E_HIP && !e.coeff.p && g_live.size() == 1);       // the bounds stay, the local went
        g_fail_at = 1;
        CHECK(like_lz_upload(e, false) == SVC_E_NOMEM && !e.coeff.p && g_live.size() == 1);
        CHECK(like_lz_upload(e, false) == SVC_OK && live(e.coeff.p) && live(e.bounds.p) && g_live.size() == 2);
        ResampleTab moved(std::move(e));
        CHECK(!e.coeff.p && !e.bounds.p && live(moved.coeff.p) && g_live.size() == 2);
    }
    CHECK(g_mallocs == g_frees && g_bad_frees == 0 && g_live.empty());

    if (g_failures || !g_live.empty() || g_mallocs != g_frees || g_bad_frees) {
        fprintf(stderr, "devbuf_harness: %d failed checks, %zu live blocks, %d allocations, %d frees, %d bad frees\n", g_failures,
                g_live.size(), g_mallocs, g_frees, g_bad_frees);
        return 1;
    }
    printf("devbuf_harness ok: %d allocations, %d frees\n", g_mallocs, g_frees);
    return 0;
}
