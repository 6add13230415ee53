// Host-only check of the engine's bookkeeping types, built with -fsanitize=address,undefined by test_host_pieces.py:
// PlanKey / GraphKey equality, CacheTag, and DeviceBuf with its three device calls swapped for malloc / free
// (SD_DEVICEBUF_HOST_ALLOC).  No GPU, no HIP call; a leak or an out-of-bounds write fails the run through the sanitizer.
#include <cstdio>
#include <cstring>

#include "../stablediffusion_amd/csrc/model.h"

using namespace sd;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// the key UNet::forward built before PlanKey: fields XORed into one long
static long old_xor_key(int B, int H, int W, int L, bool kv_cache, int ip_tokens, bool cfg_share) {
    return ((long)B << 40) ^ ((long)H << 20) ^ (long)W ^ ((long)L << 52) ^ (kv_cache ? (1L << 62) : 0) ^
           ((long)ip_tokens << 32) ^ (cfg_share ? (1L << 61) : 0);
}

static PlanKey key(int B, int H, int W, int L, int ip_tokens) {
    PlanKey k;
    k.B = B; k.H = H; k.W = W; k.L = L; k.ip_tokens = ip_tokens;
    return k;
}

static void plan_keys() {
    // H bit 12 lands on bit 32 of the old key, where the IP token count's bit 0 sits: two calls, one old key
    CHECK(old_xor_key(2, 4096 + 64, 64, 77, false, 0, false) == old_xor_key(2, 64, 64, 77, false, 1, false));
    CHECK(!(key(2, 4096 + 64, 64, 77, 0) == key(2, 64, 64, 77, 1)));
    // likewise B bit 12 against L bit 0 (bit 52)
    CHECK(old_xor_key(4096 + 2, 64, 64, 76, false, 0, false) == old_xor_key(2, 64, 64, 77, false, 0, false));
    CHECK(!(key(4096 + 2, 64, 64, 76, 0) == key(2, 64, 64, 77, 0)));
    // every field takes part
    const PlanKey a = key(2, 64, 64, 77, 4);
    PlanKey b = a;
    CHECK(a == b);
    b = a; b.kv_cache = true; CHECK(!(a == b));
    b = a; b.cfg_share = true; CHECK(!(a == b));
    b = a; b.pag_groups = 2; CHECK(!(a == b));
    b = a; b.pag_late = true; CHECK(!(a == b));
    b = a; b.n_ctrl = 1; CHECK(!(a == b));
    b = a; b.dc_depth = 1; CHECK(!(a == b));
    b = a; b.W = 32; CHECK(!(a == b));
    // one slot per DeepCache mode, as UNet::planned holds them: planning one leaves the others alone, and a reset slot
    // (UNet::reset_plans) equals no key a forward can build, since those have B > 0
    PlanKey planned[3];
    planned[SD_DC_STORE] = a;
    CHECK(!(planned[SD_DC_PLAIN] == a) && planned[SD_DC_STORE] == a && !(planned[SD_DC_REUSE] == a));
    planned[SD_DC_REUSE] = key(1, 64, 64, 77, 0);
    CHECK(planned[SD_DC_STORE] == a && planned[SD_DC_PLAIN] == PlanKey());
    for (PlanKey& k : planned) k = PlanKey();
    for (const PlanKey& k : planned) CHECK(k == PlanKey() && !(k == a) && k.B == 0);

    GraphKey g, h;
    g.B = h.B = 2; g.H = h.H = 64; g.W = h.W = 64; g.L = h.L = 77;
    CHECK(g == h && !(g == GraphKey()));
    h.tcond = true;
    CHECK(!(g == h));
}

static void cache_tags() {
    int x = 0, y = 0;
    CacheTag t;
    CHECK(!t.matches(nullptr, 0) && !t.matches(&x, 2, 77));
    t.set(&x, 2, 77, 1);
    CHECK(t.matches(&x, 2, 77, 1));
    CHECK(!t.matches(&y, 2, 77, 1) && !t.matches(&x, 1, 77, 1) && !t.matches(&x, 2, 76, 1) && !t.matches(&x, 2, 77) &&
          !t.matches(&x, 2, 77, 1, 1));
    t.clear();
    CHECK(!t.matches(&x, 2, 77, 1));
    t.set(nullptr, 2, 16, 16, 1);       // (DeepCache's: no pointer)
    CHECK(t.matches(nullptr, 2, 16, 16, 1) && !t.matches(nullptr, 2, 16, 16, 0));
}

static void device_bufs() {
    bool grew = false;
    {
        DeviceBuf b;
        CHECK(b.data() == nullptr && b.capacity() == 0);
        CHECK(b.reserve(0, &grew) == 0 && !grew && b.data() == nullptr);
        CHECK(b.reserve(100, &grew) == 0 && grew && b.data() != nullptr && b.capacity() == 100);
        std::memset(b.data(), 0x5a, 100);
        char* p = b.data();
        CHECK(b.reserve(50, &grew) == 0 && !grew && b.data() == p && b.capacity() == 100);
        CHECK(b.reserve(100, &grew) == 0 && !grew && b.data() == p);
        CHECK(b.data()[99] == 0x5a);
        CHECK(b.reserve(101, &grew) == 0 && grew && b.capacity() == 101);
        std::memset(b.data(), 1, 101);
        CHECK(b.release() == 0 && b.data() == nullptr && b.capacity() == 0);
        CHECK(b.release() == 0);
        CHECK(b.reserve(8, &grew) == 0 && grew && b.capacity() == 8);
        CHECK(reinterpret_cast<char*>(b.h()) == b.data());
    }                                   // destroyed holding 8 bytes: the leak check sees them freed
    { DeviceBuf empty; }
    DeviceBuf a, c;
    CHECK(a.reserve(16, &grew) == 0 && c.reserve(32, &grew) == 0 && a.data() != c.data());
    CHECK(a.release() == 0 && c.capacity() == 32);
}

int main() {
    plan_keys();
    cache_tags();
    device_bufs();
    if (failures) std::printf("host pieces: %d check(s) failed\n", failures);
    else std::printf("host pieces: ok\n");
    return failures ? 1 : 0;
}
