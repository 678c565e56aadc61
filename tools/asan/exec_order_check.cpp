// Host check of the executor's stream order (csrc/exec.cpp), no device: exec.cpp and
// error.cpp are linked against exec_stubs.cpp, which records every event call and launch.
// The trace is replayed with happens-before sets (a launch on stream s inherits s's set and
// joins it; record(e, s) copies s's set into e; wait(s, e) merges e's into s) and the
// ordering contract is checked on synthetic op lists and on lists read from a file:
//   exec_order_check [--trace]                       the synthetic lists
//   exec_order_check --blob FILE --nops N [--side] [--side2] [--trace]
// For a file it prints, per main-stream record, "main K: i j ..." — the list indices of the
// side records the main stream has waited for when record K launches. --trace prints the
// raw trace as well. Built by tools/asan/build.sh with -fsanitize=address,undefined.
// Exit 0, "OK: 0 failure(s)" and no sanitizer report = pass.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <string>
#include <vector>

#include "../../include/isg.h"
#include "exec_trace.h"

static int failures = 0;
static const char* g_case = "";
#define EXPECT(c, ...)                                                            \
    do {                                                                          \
        if (!(c)) {                                                               \
            std::fprintf(stderr, "FAIL [%s] %s:%d %s: ", g_case, __FILE__, __LINE__, #c); \
            std::fprintf(stderr, __VA_ARGS__);                                    \
            std::fprintf(stderr, "\n");                                           \
            ++failures;                                                           \
        }                                                                         \
    } while (0)

enum { F_SIDE = 1, F_JOIN = 2, F_FORK_NOW = 4, EXCL_SHIFT = 8, BATCH = 16 };
enum { K_WGRAD = 3, K_BN_UPDATE = 9, K_GRAD_FINAL = 10, K_MEMSET = 12, K_KP_WGRAD = 16, K_HEAD_FOLD = 22, K_STEP_INC = 25 };
static bool wgrad_kind(int k) { return k == K_WGRAD || k == K_KP_WGRAD || k == K_HEAD_FOLD; }
static bool spread_kind(int k) { return wgrad_kind(k) || k == K_GRAD_FINAL || k == K_BN_UPDATE || k == K_STEP_INC; }

static isg_stream_t stream(int i) { return (isg_stream_t)(uintptr_t)i; }
enum { SLOTS = 4096 };
static void* g_table[SLOTS];

struct Rec {
    int kind, flags;
    uint64_t id;
    int key;
};
typedef std::vector<char> Blob;

// ---- the program's own parse: record boundaries, then each record's identity as the
// stubs see it (the record alone through isg_exec) ------------------------------------
static bool parse(const Blob& b, int nops, std::vector<Rec>* out) {
    size_t p = 0;
    for (int i = 0; i < nops; ++i) {
        int32_t h[4];
        if (p + sizeof(h) > b.size()) return false;
        std::memcpy(h, b.data() + p, sizeof(h));
        if (h[1] < 0 || h[1] > 8192 || h[2] < 0) return false;
        const size_t len = sizeof(h) + (size_t)((h[1] + 7) & ~7) + 16 * (size_t)h[2];
        if (p + len > b.size()) return false;
        for (int f = 0; f < h[2]; ++f) {
            int32_t ls[2];
            std::memcpy(ls, b.data() + p + sizeof(h) + ((h[1] + 7) & ~7) + 16 * f, sizeof(ls));
            if (ls[0] < 0 || ls[0] + 8 > h[1] || ls[1] >= SLOTS) return false;
        }
        Blob one(b.begin() + p, b.begin() + p + len);
        int32_t zero = 0;
        std::memcpy(one.data() + 12, &zero, 4);  // no flags
        g_trace.clear();
        if (isg_exec(one.data(), 1, g_table, stream(1)) != ISG_OK || g_trace.size() != 1) return false;
        out->push_back({h[0], h[3], g_trace[0].members[0].id, g_trace[0].members[0].key});
        p += len;
    }
    return true;
}

// ---- happens-before sets over list indices ------------------------------------------------
struct Bits {
    std::vector<uint64_t> w;
    explicit Bits(size_t n = 0) : w((n + 63) / 64, 0) {}
    void set(int i) { w[i / 64] |= 1ull << (i % 64); }
    bool has(int i) const { return w[i / 64] >> (i % 64) & 1; }
    void merge(const Bits& o) { for (size_t i = 0; i < w.size(); ++i) w[i] |= o.w[i]; }
};

struct Replay {
    std::vector<Bits> before;        // per record: its stream's set when it launched
    std::vector<int> pos, st, batch; // per record: trace position, stream, fork number (-1 main)
    std::vector<std::vector<int>> launches;  // per trace entry: the records it launched
    int nbatch = 0;
    Bits final_main;
};

// maps the trace's launches to list indices and replays it; false when a launch is no record
// of the list (or one launched twice). Properties 4 and 8 (exactly once).
static bool replay(const std::vector<Rec>& recs, bool side, Replay* r) {
    const int n = (int)recs.size();
    std::deque<int> mains;
    std::map<uint64_t, std::deque<int>> sides;
    for (int i = 0; i < n; ++i) {
        if (side && (recs[i].flags & F_SIDE)) sides[recs[i].id ^ (uint64_t)recs[i].kind << 56].push_back(i);
        else mains.push_back(i);
    }
    Bits S[4] = {Bits(n), Bits(n), Bits(n), Bits(n)};
    std::map<int, Bits> E;
    r->before.assign(n, Bits(n));
    r->pos.assign(n, -1);
    r->st.assign(n, 0);
    r->batch.assign(n, -1);
    r->launches.assign(g_trace.size(), {});
    int fork = -1;
    for (size_t t = 0; t < g_trace.size(); ++t) {
        const TraceEntry& e = g_trace[t];
        if (e.stream < 0 || e.stream > 3) return false;
        if (e.type == TraceEntry::RECORD) {
            E[e.event] = S[e.stream];
            if (e.stream == 1) ++fork;
        } else if (e.type == TraceEntry::WAIT) {
            if (!E.count(e.event)) return false;  // waits for an event never recorded
            S[e.stream].merge(E[e.event]);
        } else if (e.type == TraceEntry::LAUNCH || e.type == TraceEntry::GROUP) {
            for (const TraceMember& m : e.members) {
                int i;
                if (e.stream == 1) {
                    if (mains.empty() || recs[mains.front()].id != m.id || recs[mains.front()].kind != e.kind) {
                        EXPECT(false, "main-stream launch %zu is not the next main-stream record", t);
                        return false;
                    }
                    i = mains.front();
                    mains.pop_front();
                } else {
                    auto& q = sides[m.id ^ (uint64_t)e.kind << 56];
                    if (q.empty()) {
                        EXPECT(false, "side launch %zu is no unlaunched side record", t);
                        return false;
                    }
                    i = q.front();
                    q.pop_front();
                    r->batch[i] = fork;
                }
                r->before[i] = S[e.stream];
                r->pos[i] = (int)t;
                r->st[i] = e.stream;
                r->launches[t].push_back(i);
            }
            for (int i : r->launches[t]) S[e.stream].set(i);
        }
    }
    r->nbatch = fork + 1;
    r->final_main = S[1];
    return true;
}

// the ordering contract on a complete (error-free) run; g_trace holds the run's trace
static void check(const std::vector<Rec>& recs, bool side, bool side2, Replay* out = nullptr) {
    const int n = (int)recs.size();
    const int failed_before = failures;
    Replay r;
    if (!replay(recs, side, &r)) return;
    for (int i = 0; i < n; ++i) EXPECT(r.pos[i] >= 0, "record %d never launched", i);  // 8
    if (failures > failed_before) return;
    auto is_side = [&](int i) { return side && (recs[i].flags & F_SIDE); };
    // 6: no side stream -> main only, no event call; one side stream -> nothing on stream 3
    for (const TraceEntry& e : g_trace) {
        if (!side) EXPECT((e.type == TraceEntry::LAUNCH) && e.stream == 1, "event call or side launch without a side stream");
        if (!side2) EXPECT(e.stream != 3, "stream 3 touched without side 2");
    }
    std::vector<int> side_idx;  // list indices of the side records so far
    std::vector<int> full_joins;
    for (int k = 0; k < n; ++k) {
        // 1: a side record runs after every earlier main-stream record
        if (is_side(k))
            for (int m = 0; m < k; ++m)
                if (!is_side(m)) EXPECT(r.before[k].has(m), "side record %d not after main record %d", k, m);
        // 2: joins
        if (side && (recs[k].flags & F_JOIN)) {
            const int ns = (int)side_idx.size(), e = recs[k].flags >> EXCL_SHIFT;
            const bool partial = e > 0 && e <= ns;
            if (!partial) full_joins.push_back(k);
            for (int j = 0; j < (partial ? ns - e : ns); ++j)
                EXPECT(r.before[k].has(side_idx[j]), "join record %d (excl %d) not after side record %d", k, e, side_idx[j]);
        }
        if (is_side(k)) side_idx.push_back(k);
    }
    // 3: the final join
    for (int i = 0; i < n; ++i) EXPECT(r.final_main.has(i), "main stream does not hold record %d on return", i);
    // 5, 7, 8: batches
    std::vector<std::vector<int>> batches(r.nbatch);
    for (int i : side_idx) {
        EXPECT(r.batch[i] >= 0, "side record %d launched before any fork", i);
        if (r.batch[i] >= 0) batches[r.batch[i]].push_back(i);
    }
    if (failures > failed_before) return;
    for (size_t s = 0; s + 1 < side_idx.size(); ++s)  // batches hold consecutive side records in order
        EXPECT(r.batch[side_idx[s]] <= r.batch[side_idx[s + 1]], "side records %d, %d forked out of order", side_idx[s], side_idx[s + 1]);
    for (int k = 0; k < n; ++k) {
        if (!is_side(k) || !(recs[k].flags & F_FORK_NOW)) continue;
        int m = k + 1;
        while (m < n && is_side(m)) ++m;
        if (m < n) EXPECT(r.pos[k] < r.pos[m], "FORK_NOW record %d issued after main record %d", k, m);
        // consecutive forked records share a fork unless the batch was full
        if (k + 1 < n && is_side(k + 1) && (recs[k + 1].flags & F_FORK_NOW) && !(recs[k + 1].flags & F_JOIN) &&
            !(batches[r.batch[k]].size() == BATCH && batches[r.batch[k]].back() == k))
            EXPECT(r.batch[k] == r.batch[k + 1], "forked records %d, %d do not share a fork event", k, k + 1);
    }
    Bits on3(n);  // everything launched on stream 3 so far
    for (const std::vector<int>& b : batches) {
        EXPECT(!b.empty() && b.size() <= BATCH, "a batch of %zu records", b.size());
        if (b.empty()) continue;
        bool all_spread = true, all_wgrad = true, uses3 = false;
        for (int i : b) {
            all_spread = all_spread && spread_kind(recs[i].kind);
            all_wgrad = all_wgrad && wgrad_kind(recs[i].kind);
            uses3 = uses3 || r.st[i] == 3;
        }
        // 7: only batches of the weight-gradient class are spread; another one runs after side
        // 2's outstanding records, and the batches behind it stay on `side` up to the next full join
        EXPECT(!uses3 || all_spread, "batch at record %d spread with a record outside the class", b[0]);
        if (side2 && !all_spread) {
            for (int i : b)
                for (int j = 0; j < n; ++j)
                    if (on3.has(j)) EXPECT(r.before[i].has(j), "record %d not after side-2 record %d", i, j);
            auto fj = std::upper_bound(full_joins.begin(), full_joins.end(), b.back());
            const int upto = fj == full_joins.end() ? n : *fj;
            for (int i = b.back() + 1; i < upto; ++i)
                if (is_side(i)) EXPECT(r.st[i] == 2, "record %d on side 2 behind a side-only batch", i);
        }
        for (int i : b)
            if (r.st[i] == 3) on3.set(i);
        // 8: grouping
        int last_first = -1;
        int t0 = r.pos[b[0]], t1 = t0;
        for (int i : b) t0 = std::min(t0, r.pos[i]), t1 = std::max(t1, r.pos[i]);
        for (int t = t0; t <= t1; ++t) {
            const std::vector<int>& l = r.launches[t];
            if (l.empty()) continue;
            const TraceEntry& e = g_trace[t];
            EXPECT(l[0] > last_first, "launch of record %d before its place", l[0]);
            last_first = l[0];
            if (e.type != TraceEntry::GROUP) {
                EXPECT(!(all_wgrad && recs[l[0]].key > 0), "record %d (key %d) launched outside a group", l[0], recs[l[0]].key);
                continue;
            }
            EXPECT(all_wgrad, "a group in the mixed batch at record %d", b[0]);
            EXPECT((int)l.size() <= std::min(g_group_max, 8) && std::is_sorted(l.begin(), l.end()), "group at record %d: %zu members", l[0], l.size());
            for (const TraceMember& m : e.members) EXPECT(m.key == e.members[0].key && m.key > 0, "group at record %d mixes keys", l[0]);
        }
    }
    if (out) *out = r;
}

// ---- synthetic lists --------------------------------------------------------------------------
struct MemsetRec { void* p; int64_t bytes; };
struct StepIncRec { int32_t* step; };
struct WgradRec {
    isg_conv_geom g;
    isg_vtensor dy, x;
    double *dw, *dbias;
    int64_t rep_stride;
    int32_t nrep, pad_;
};
struct ListRec { int32_t n, pad_; };

struct List {
    Blob b;
    int nops = 0;
    uintptr_t tag = 0x1000;  // every record's payload differs
    void put(int kind, const void* desc, int bytes, int flags, int fix_loc = -1) {
        const int32_t h[4] = {kind, bytes, fix_loc >= 0 ? 1 : 0, flags};
        b.insert(b.end(), (const char*)h, (const char*)h + sizeof(h));
        b.insert(b.end(), (const char*)desc, (const char*)desc + bytes);
        b.resize(b.size() + (8 - bytes % 8) % 8, 0);
        if (fix_loc >= 0) {
            const int32_t lf[2] = {fix_loc, 3};
            const int64_t off = (int64_t)(tag += 16);
            b.insert(b.end(), (const char*)lf, (const char*)lf + sizeof(lf));
            b.insert(b.end(), (const char*)&off, (const char*)&off + 8);
        }
        ++nops;
    }
    void memset(int flags) { MemsetRec m{nullptr, 64}; put(K_MEMSET, &m, sizeof(m), flags, 0); }  // pointer by fix-up
    void step_inc(int flags) { StepIncRec s{(int32_t*)(tag += 16)}; put(K_STEP_INC, &s, sizeof(s), flags); }
    void wgrad(int flags, int co, int k) {  // k == 1: the stub's isg_pwg_plan keys it by co
        WgradRec w{};
        w.g.N = w.g.Ci = 1; w.g.Co = co; w.g.H = w.g.W = w.g.OH = w.g.OW = 4; w.g.KH = w.g.KW = k;
        w.g.SH = w.g.SW = w.g.DH = w.g.DW = 1; w.g.PH = w.g.PW = k / 2; w.g.groups = 1;
        w.dw = (double*)(tag += 16); w.nrep = 1;
        put(K_WGRAD, &w, sizeof(w), flags);
    }
    void kp_wgrad(int flags) {
        isg_kp_stem a{};
        tag += 16;
        std::memcpy(&a, &tag, sizeof(tag));
        put(K_KP_WGRAD, &a, sizeof(a), flags);
    }
    void grad_final(int flags) {
        char d[sizeof(ListRec) + sizeof(isg_grad_final)] = {};
        const ListRec l{1, 0};
        tag += 16;
        std::memcpy(d, &l, sizeof(l));
        std::memcpy(d + sizeof(l), &tag, sizeof(tag));
        put(K_GRAD_FINAL, d, sizeof(d), flags);
    }
    // which: 0 memset, 1 step counter, 2 3x3 weight gradient, 3 stem weight gradient,
    // 4 gradient finalisation, 5.. 1x1 weight gradients of three keys
    static int kind_of(int which) { return which == 0 ? K_MEMSET : which == 1 ? K_STEP_INC : which == 3 ? K_KP_WGRAD : which == 4 ? K_GRAD_FINAL : K_WGRAD; }
    void any(int which, int flags) {
        switch (which) {
            case 0: memset(flags); break;
            case 1: step_inc(flags); break;
            case 2: wgrad(flags, 8, 3); break;
            case 3: kp_wgrad(flags); break;
            case 4: grad_final(flags); break;
            default: wgrad(flags, 8 * (which - 4), 1); break;
        }
    }
};

static uint32_t g_rng = 12345;
static int rnd(int n) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (int)((g_rng >> 8) % (uint32_t)n);
}

static bool g_print_trace = false;
static int32_t run(const List& l, bool side, bool side2) {
    g_trace.clear();
    const int32_t rc = isg_exec_ms2(l.b.data(), l.nops, g_table, stream(1), side ? stream(2) : nullptr,
                                    side2 ? stream(3) : nullptr);
    if (g_print_trace) {
        std::printf("# %s side %d side2 %d gmax %d: rc %d\n", g_case, side, side2, g_group_max, rc);
        for (const TraceEntry& e : g_trace) trace_print(e);
    }
    return rc;
}

// the list under no, one and two side streams
static void check_list(const char* name, const List& l) {
    g_case = name;
    std::vector<Rec> recs;
    if (!parse(l.b, l.nops, &recs)) {
        EXPECT(false, "the list does not parse");
        return;
    }
    for (int mode = 0; mode < 3; ++mode) {
        const int32_t rc = run(l, mode >= 1, mode == 2);
        EXPECT(rc == ISG_OK, "rc %d (%s)", rc, isg_last_error());
        if (rc == ISG_OK) check(recs, mode >= 1, mode == 2);
    }
}

// side records with probability side_pct, of the kinds below `kinds`; joins full and partial,
// with exclusion counts up to two past the side records so far
static List random_list(int n, int side_pct, int kinds, int join_pct) {
    List l;
    int nside = 0;
    for (int i = 0; i < n; ++i) {
        int flags = 0;
        if (rnd(100) < side_pct) flags |= F_SIDE | (rnd(2) ? F_FORK_NOW : 0);
        if (rnd(100) < join_pct) flags |= F_JOIN | (rnd(3) ? rnd(nside + 3) << EXCL_SHIFT : 0);
        l.any(flags & F_SIDE ? rnd(kinds) : rnd(2) * 2, flags);
        nside += flags & F_SIDE ? 1 : 0;
    }
    return l;
}

static void synthetic() {
    char name[64];
    for (int t = 0; t < 60; ++t) {
        std::snprintf(name, sizeof(name), "random %d", t);
        g_group_max = 1 + rnd(12);
        // thirds: any kind; the weight-gradient class only (spread batches); weight gradients only (groups)
        check_list(name, random_list(20 + rnd(120), 30 + rnd(60), t % 3 == 0 ? 8 : 1 + t % 3 * 3, rnd(25)));
    }
    g_group_max = 4;
    {   // more than 64 batches of 16: both event pools wrap; partial joins into old batches
        List l;
        for (int i = 0; i < 1500; ++i) {
            const bool side = i % 4 != 0;
            int flags = side ? F_SIDE : 0;
            if (i % 97 == 0) flags |= F_JOIN | (i % 2 ? (1 + rnd(40)) << EXCL_SHIFT : 0);
            if (i > 1200 && i % 50 == 1) flags |= F_JOIN | (1000 + rnd(100)) << EXCL_SHIFT;  // far back: a reused event
            l.any(side ? 1 + rnd(7) : 0, flags);
        }
        check_list("pools wrap", l);
    }
    {   // a join that excludes more side records than there are: a full join
        List l;
        l.memset(0); l.wgrad(F_SIDE, 8, 1); l.wgrad(F_SIDE, 8, 1); l.memset(F_JOIN | 3 << EXCL_SHIFT);
        l.step_inc(F_SIDE); l.memset(F_JOIN | 1 << EXCL_SHIFT); l.memset(F_JOIN | 3 << EXCL_SHIFT);
        check_list("join past nside", l);
    }
    {   // a FORK_NOW record last in the list
        List l;
        l.memset(0); l.wgrad(F_SIDE, 8, 1); l.memset(0); l.kp_wgrad(F_SIDE | F_FORK_NOW);
        check_list("fork-now last", l);
    }
    {   // side records only
        List l;
        for (int i = 0; i < 40; ++i) l.any(1 + i % 7, F_SIDE | (i % 5 == 0 ? F_FORK_NOW : 0));
        check_list("side only", l);
    }
    {   // side 2: spread batches, a side-only batch behind them, spread batches behind that (serial)
        List l;
        for (int i = 0; i < 20; ++i) l.wgrad(F_SIDE, 8 + 8 * (i % 2), 1);
        l.memset(F_SIDE | F_FORK_NOW); l.memset(0);
        for (int i = 0; i < 20; ++i) l.wgrad(F_SIDE, 8, 1 + 2 * (i % 2));
        l.memset(F_JOIN);
        for (int i = 0; i < 20; ++i) l.any(1 + i % 7, F_SIDE);
        check_list("side 2 serial", l);
    }
}

// ---- errors (the executor's own, whatever the stubs do) ------------------------------------
static void errors() {
    g_case = "errors";
    List l;
    for (int i = 0; i < 40; ++i) l.any(i % 8, i % 3 == 1 ? F_SIDE : 0);
    char want[64];
    for (int side = 0; side < 2; ++side)
        for (int at : {1, 7, 40}) {
            g_fail_at = at;
            const int32_t rc = run(l, side, false);
            g_fail_at = 0;
            EXPECT(rc == ISG_ERR_HIP, "rc %d", rc);
            EXPECT(!g_trace.empty() && g_trace.back().failed, "a call after the failing launch");
            if (side) continue;  // (with a side stream the failing launch is not the current record's)
            std::snprintf(want, sizeof(want), "exec op %d (kind %d)", at - 1, List::kind_of((at - 1) % 8));
            EXPECT(std::strstr(isg_last_error(), want), "'%s' lacks '%s'", isg_last_error(), want);
        }
    {   // a full side batch whose first launch fails: reported at the record that closed it
        List s;
        for (int i = 0; i < BATCH; ++i) s.memset(F_SIDE);
        s.memset(0);
        g_fail_at = 1;
        const int32_t rc = run(s, true, false);
        g_fail_at = 0;
        EXPECT(rc == ISG_ERR_HIP && std::strstr(isg_last_error(), "exec op 15 (kind 12)"), "rc %d '%s'", rc, isg_last_error());
        EXPECT(g_trace.back().failed, "a call after the failing launch");
    }
    for (int32_t bytes : {-1, 8193}) {
        List b;
        b.memset(0);
        std::memcpy(b.b.data() + 4, &bytes, 4);
        b.b.resize(16384, 0);
        EXPECT(run(b, false, false) == ISG_ERR_INVALID && std::strstr(isg_last_error(), "bad desc size"), "'%s'", isg_last_error());
        EXPECT(g_trace.empty(), "a launch of a malformed record");
    }
    List u;
    u.memset(0);
    const int32_t kind = 77;
    std::memcpy(u.b.data(), &kind, 4);
    EXPECT(run(u, true, false) == ISG_ERR_INVALID && std::strstr(isg_last_error(), "unknown op kind 77"), "'%s'", isg_last_error());
}

static int blob_mode(const char* file, int nops, bool side, bool side2) {
    g_case = file;
    FILE* f = std::fopen(file, "rb");
    if (!f) return std::fprintf(stderr, "cannot open %s\n", file), 2;
    List l;
    char chunk[65536];
    for (size_t k; (k = std::fread(chunk, 1, sizeof(chunk), f)) > 0;) l.b.insert(l.b.end(), chunk, chunk + k);
    std::fclose(f);
    l.nops = nops;
    std::vector<Rec> recs;
    if (!parse(l.b, nops, &recs)) return std::fprintf(stderr, "%s does not parse as %d records\n", file, nops), 2;
    const int32_t rc = run(l, side, side2);
    EXPECT(rc == ISG_OK, "rc %d (%s)", rc, isg_last_error());
    Replay r;
    if (rc == ISG_OK) check(recs, side, side2, &r);
    if (r.before.empty()) return 1;
    for (int k = 0; k < nops; ++k) {
        if (side && (recs[k].flags & F_SIDE)) continue;
        std::printf("main %d:", k);
        for (int i = 0; i < nops; ++i)
            if (side && (recs[i].flags & F_SIDE) && r.before[k].has(i)) std::printf(" %d", i);
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    const char* file = nullptr;
    int nops = 0;
    bool side = false, side2 = false;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--trace")) g_print_trace = true;
        else if (!std::strcmp(argv[i], "--side")) side = true;
        else if (!std::strcmp(argv[i], "--side2")) side = side2 = true;
        else if (!std::strcmp(argv[i], "--blob") && i + 1 < argc) file = argv[++i];
        else if (!std::strcmp(argv[i], "--nops") && i + 1 < argc) nops = std::atoi(argv[++i]);
        else return std::fprintf(stderr, "usage: exec_order_check [--trace] [--blob FILE --nops N [--side] [--side2]]\n"), 2;
    }
    for (int i = 0; i < SLOTS; ++i) g_table[i] = (void*)((uintptr_t)(i + 1) << 40);  // never dereferenced
    if (file) {
        if (int e = blob_mode(file, nops, side, side2)) return e;
    } else {
        synthetic();
        errors();
    }
    std::printf("%s: %d failure(s)\n", failures ? "FAIL" : "OK", failures);
    return failures ? 1 : 0;
}
