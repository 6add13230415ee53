// Host-only check of the engine's bookkeeping types, built with -fsanitize=address,undefined by test_host_pieces.py:
// PlanKey / GraphKey equality, the graph replay decision (graph_may_replay), CacheTag, and DeviceBuf with its three device calls swapped for malloc / free
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

// graph_may_replay: the one place that says whether UNet::forward_graph launches its captured graph or captures again
static void graph_replay_decision() {
    char arena_a[64], arena_b[64], io_a[16], io_b[16];      // stand-ins for the slabs: only their addresses are used
    GraphKey k;
    k.B = 2; k.H = 8; k.W = 8; k.L = 77;
    const GraphDeps d{arena_a, 4096, io_a};
    // same key, nothing moved: replay
    CHECK(graph_may_replay(k, d, k, d, true));
    // every key field, one at a time: capture
    GraphKey o;
    o = k; o.B = 1; CHECK(!graph_may_replay(o, d, k, d, true));
    o = k; o.H = 16; CHECK(!graph_may_replay(o, d, k, d, true));
    o = k; o.W = 16; CHECK(!graph_may_replay(o, d, k, d, true));
    o = k; o.L = 32; CHECK(!graph_may_replay(o, d, k, d, true));
    o = k; o.tcond = true; CHECK(!graph_may_replay(o, d, k, d, true));
    // (H and W swapped is another key)
    GraphKey hw = k, wh = k;
    hw.H = 24; hw.W = 16; wh.H = 16; wh.W = 24;
    CHECK(!graph_may_replay(hw, d, wh, d, true) && graph_may_replay(hw, d, hw, d, true));
    // arena regrown with the same key: another slab, or -- the allocator handing the old address out again -- the same
    // address with another capacity
    GraphDeps n = d;
    n.arena_base = arena_b; n.arena_cap = 8192; CHECK(!graph_may_replay(k, n, k, d, true));
    n = d; n.arena_cap = 8192; CHECK(!graph_may_replay(k, n, k, d, true));
    n = d; n.arena_base = arena_b; CHECK(!graph_may_replay(k, n, k, d, true));
    // staging slab regrown
    n = d; n.io_base = io_b; CHECK(!graph_may_replay(k, n, k, d, true));
    // no executable (never captured, or the last capture failed), whatever else agrees
    CHECK(!graph_may_replay(k, d, k, d, false));
    CHECK(!graph_may_replay(GraphKey(), GraphDeps(), GraphKey(), GraphDeps(), false));
    // what forward_graph does after a capture -- remember the key and the slabs as they are then -- makes the next
    // call with that key a replay, and the one after a regrowth a capture
    GraphKey captured_key;
    GraphDeps captured;
    bool have = false;
    CHECK(!graph_may_replay(k, d, captured_key, captured, have));
    captured_key = k; captured = GraphDeps{arena_b, 8192, io_a}; have = true;   // (the capturing call grew the arena itself)
    const GraphDeps after{arena_b, 8192, io_a};
    CHECK(graph_may_replay(k, after, captured_key, captured, have));
    const GraphDeps regrown{arena_a, 16384, io_a};
    CHECK(!graph_may_replay(k, regrown, captured_key, captured, have));
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
    graph_replay_decision();
    cache_tags();
    device_bufs();
    if (failures) std::printf("host pieces: %d check(s) failed\n", failures);
    else std::printf("host pieces: ok\n");
    return failures ? 1 : 0;
}
