// Host-side AddressSanitizer check of libisg's C-ABI (SURVEY.md §5 "sanitizers": GPU ASan
// is not available on this pool, so the host half runs instrumented on the CPU).
//
// Built by tools/asan/build.sh from every libisg source compiled host-only
// (-Xarch_host -fsanitize=address, host half only): no device code, no GPU needed. It drives the
// paths whose memory handling is host code — argument validation, the error plumbing,
// the executor's record parsing and pointer fix-ups, the chunking of host item arrays —
// with valid and malformed inputs; kernel launches fail cleanly without a device. The
// launchers' host predicates (csrc/launch.h, stage.h's fast ones) are driven directly on
// host structs. The executor cases here cover record parsing only: which stream and which
// event every record gets is checked by exec_order_check.cpp, next to this file.
// Exit 0 and no ASan report = pass.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/isg.h"
#include "../../instancesegmentation_amd/csrc/stage.h"  // launch.h's predicates + the fast ones

static int failures = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// executor blob: header {kind, desc_bytes, nfix, flags}, desc (8-aligned), fixes
static void put_op(std::vector<char>& b, int kind, const void* desc, int bytes,
                   const std::vector<isg_ref>& fix, const std::vector<int>& locs, int flags = 0) {
    int32_t h[4] = {kind, bytes, (int32_t)fix.size(), flags};
    b.insert(b.end(), (char*)h, (char*)h + sizeof(h));
    b.insert(b.end(), (const char*)desc, (const char*)desc + bytes);
    b.resize(b.size() + ((8 - bytes % 8) % 8), 0);
    for (size_t i = 0; i < fix.size(); ++i) {
        int32_t lf[2] = {locs[i], fix[i].slot};
        b.insert(b.end(), (char*)lf, (char*)lf + sizeof(lf));
        b.insert(b.end(), (const char*)&fix[i].offset, (const char*)&fix[i].offset + 8);
    }
}

// csrc/launch.h: the predicates that pick a kernel and its template flags, on host structs
static void check_launch_predicates() {
    alignas(16) static float buf[64];
    float* const ok = buf;
    float* const off4 = buf + 1;  // 4 bytes off a 16-B boundary
    EXPECT(aligned16(ok) && aligned16(nullptr) && !aligned16(off4));

    isg_vtensor v{};
    v.nseg = 2;
    v.s[0].p = ok; v.s[0].n_stride = 64; v.s[0].C = 4;
    v.s[1].p = ok + 4; v.s[1].n_stride = 128; v.s[1].C = 3;
    EXPECT(vt_rows16(v) && vt_channels(&v) == 7);
    { isg_vtensor t = v; t.s[1].p = off4; EXPECT(!vt_rows16(t)); }
    { isg_vtensor t = v; t.s[0].n_stride = 65; EXPECT(!vt_rows16(t)); }  // n_stride % 4 == 1
    {   // a BN_BWD y misaligned while p is aligned; y's stride; a NULL y has nothing to check
        isg_vtensor t = v;
        t.s[0].xform = ISG_XF_BN_BWD; t.s[0].y = off4; t.s[0].y_n_stride = 64;
        EXPECT(!vt_rows16(t));
        t.s[0].y = ok; t.s[0].y_n_stride = 66;
        EXPECT(!vt_rows16(t));
        t.s[0].y_n_stride = 64;
        EXPECT(vt_rows16(t));
        t.s[0].y = nullptr; t.s[0].y_n_stride = 1;
        EXPECT(vt_rows16(t));
        t.s[0].xform = ISG_XF_PLAIN; t.s[0].y = off4;  // a PLAIN segment's y is not an operand
        EXPECT(vt_rows16(t));
    }
    {   // the residual forms: a BN_FWD y and a mat
        isg_vtensor t = v;
        t.s[1].xform = ISG_XF_BN_FWD; t.s[1].y = off4; t.s[1].y_n_stride = 64;
        EXPECT(!vt_rows16(t) && isg_vt_res(&t));
        t.s[1].y = ok;
        EXPECT(vt_rows16(t));
        t.mat = off4; t.mat_n_stride = 64;
        EXPECT(!vt_rows16(t));
        t.mat = ok; t.mat_n_stride = 6;
        EXPECT(!vt_rows16(t));
        t.mat_n_stride = 8;
        EXPECT(vt_rows16(t));
    }
    {   // BN_BWD without y resolves to p at p's stride
        isg_vtensor t = v;
        t.s[0].xform = ISG_XF_BN_BWD;
        const isg_vtensor r = isg_resolve_y(&t);
        EXPECT(r.s[0].y == ok && r.s[0].y_n_stride == 64 && r.s[1].y == nullptr);
        EXPECT(vt_rows16(r) == vt_rows16(t));
    }

    isg_sinks k{};
    k.nsink = 2;
    k.s[0].mode = ISG_SINK_STORE; k.s[0].p = ok; k.s[0].n_stride = 64;
    k.s[1].mode = ISG_SINK_NONE; k.s[1].p = (float*)(uintptr_t)0x1235; k.s[1].n_stride = 7;  // ignored
    EXPECT(sinks_rows16(k) && !sinks_read_operand(k) && !sinks_stat_on(k));
    { isg_sinks t = k; t.s[0].p = off4; EXPECT(!sinks_rows16(t)); }
    { isg_sinks t = k; t.s[0].n_stride = 61; EXPECT(!sinks_rows16(t)); }
    { isg_sinks t = k; t.s[0].mode = ISG_SINK_ACCUM; EXPECT(sinks_rows16(t) && sinks_read_operand(t)); }
    {   // an ACTBWD sink with y misaligned
        isg_sinks t = k;
        t.s[1].mode = ISG_SINK_ACTBWD; t.s[1].p = ok; t.s[1].n_stride = 64;
        t.s[1].y = off4; t.s[1].y_n_stride = 64;
        EXPECT(!sinks_rows16(t) && sinks_read_operand(t));
        t.s[1].y = ok; t.s[1].y_n_stride = 62;
        EXPECT(!sinks_rows16(t));
        t.s[1].y_n_stride = 64;
        EXPECT(sinks_rows16(t));
    }

    // stat_on: coef set, only stats, neither; fast: coef or training mode
    static double stats[16];
    {
        isg_vtensor t = v;
        t.s[1].xform = ISG_XF_BN_FWD;
        EXPECT(!vt_stat_on(t) && !vt_fast(t));  // neither, eval mode (train == 0): the slow path
        t.s[1].bn.train = 1;
        EXPECT(!vt_stat_on(t) && vt_fast(t));
        t.s[1].bn.stats = stats;
        EXPECT(vt_stat_on(t) && vt_fast(t));
        t.s[1].bn.train = 0;
        EXPECT(vt_stat_on(t) && !vt_fast(t));
        t.s[1].bn.coef = ok;
        EXPECT(!vt_stat_on(t) && vt_fast(t));
        t.s[1].xform = ISG_XF_PLAIN;  // no BatchNorm: its bn record is not read
        t.s[1].bn.coef = nullptr;
        EXPECT(!vt_stat_on(t) && vt_fast(t));
        t.nseg = 1;
        t.s[1].xform = ISG_XF_BN_BWD;  // past nseg
        EXPECT(vt_fast(t) && !vt_stat_on(t));
    }
    {
        isg_sinks t = k;
        t.s[0].mode = ISG_SINK_ACTBWD; t.s[0].y = ok;
        EXPECT(!sinks_stat_on(t) && !sinks_fast(t));
        t.s[0].bn.stats = stats;
        EXPECT(sinks_stat_on(t) && !sinks_fast(t));
        t.s[0].bn.train = 1;
        EXPECT(sinks_stat_on(t) && sinks_fast(t));
        t.s[0].bn.coef = ok; t.s[0].bn.train = 0;
        EXPECT(!sinks_stat_on(t) && sinks_fast(t));
        t.s[0].mode = ISG_SINK_STORE; t.s[0].bn.coef = nullptr;
        EXPECT(!sinks_stat_on(t) && sinks_fast(t));
    }

    const int want[9] = {1, 2, 3, 4, 6, 6, 8, 8, 8};
    for (int t = 1; t <= 9; ++t)
        EXPECT(with_tpw(t, [](auto T) { return (int)decltype(T)::value; }) == want[t - 1]);

    // the geometry predicates: one true case, then each field flipped in turn
    isg_conv_geom p{};
    p.N = 2; p.Ci = 8; p.Co = 8; p.H = p.OH = 6; p.W = p.OW = 10; p.KH = p.KW = 1; p.SH = p.SW = 1;
    p.DH = p.DW = 1; p.groups = 1;
    EXPECT(geom_1x1_s1(&p));
    for (int32_t isg_conv_geom::*f : {&isg_conv_geom::KH, &isg_conv_geom::KW, &isg_conv_geom::SH,
                                      &isg_conv_geom::SW, &isg_conv_geom::PH, &isg_conv_geom::PW}) {
        isg_conv_geom q = p;
        q.*f += 1;
        EXPECT(!geom_1x1_s1(&q));
    }
    isg_conv_geom d{};
    d.N = 1; d.Ci = 3; d.Co = 16; d.H = 12; d.W = 16; d.OH = 6; d.OW = 8; d.KH = d.KW = 5;
    d.SH = d.SW = 2; d.PH = d.PW = 2; d.DH = d.DW = 1; d.groups = 1; d.w_ci = 20;
    EXPECT(geom_s2k5(&d));
    for (int32_t isg_conv_geom::*f : {&isg_conv_geom::KH, &isg_conv_geom::KW, &isg_conv_geom::SH,
                                      &isg_conv_geom::SW, &isg_conv_geom::PH, &isg_conv_geom::PW,
                                      &isg_conv_geom::DH, &isg_conv_geom::DW, &isg_conv_geom::H,
                                      &isg_conv_geom::W, &isg_conv_geom::OH, &isg_conv_geom::OW,
                                      &isg_conv_geom::groups}) {
        isg_conv_geom q = d;
        q.*f += 1;
        EXPECT(!geom_s2k5(&q));
    }

    int64_t rs = 100;
    int32_t nr = 1;
    norm_replicas(rs, nr);
    EXPECT(rs == 0 && nr == 1);
    rs = 100; nr = 0;
    norm_replicas(rs, nr);
    EXPECT(rs == 0 && nr == 1);
    rs = 100; nr = 4;
    norm_replicas(rs, nr);
    EXPECT(rs == 100 && nr == 4);
    EXPECT(launched(0) == 1 && launched(ISG_ERR_HIP) == ISG_ERR_HIP);
    EXPECT(isg_cu_count() >= 1 && isg_cu_count() == isg_cu_count());  // 256 without a device
}

int main() {
    check_launch_predicates();
    EXPECT(isg_abi_version() > 0);
    EXPECT(isg_stat_replicas() == ISG_STAT_REP);
    for (int i = 0; i <= 16; ++i) EXPECT(isg_record_size(i) > 0);
    EXPECT(isg_record_size(-1) == -1 && isg_record_size(99) == -1);

    // argument validation and the thread-local message
    isg_conv_geom g{};
    EXPECT(isg_conv_fwd(nullptr, nullptr, nullptr, nullptr, nullptr) == ISG_ERR_INVALID);
    EXPECT(std::strlen(isg_last_error()) > 0);
    g.N = 1; g.Ci = 4; g.H = 8; g.W = 8; g.Co = 4; g.OH = 9; g.OW = 8;
    g.KH = g.KW = 3; g.SH = g.SW = 1; g.PH = g.PW = 1; g.DH = g.DW = 1; g.groups = 1;
    EXPECT(isg_conv_fwd(&g, nullptr, nullptr, nullptr, nullptr) == ISG_ERR_INVALID);  // OH
    g.OH = 8;
    g.groups = 2;
    EXPECT(isg_conv_dgrad(&g, nullptr, nullptr, nullptr, nullptr) == ISG_ERR_UNSUPPORTED);
    g.groups = 1;
    EXPECT(isg_conv_wgrad_rep(&g, nullptr, nullptr, nullptr, nullptr, 0, 4, nullptr) == ISG_ERR_INVALID);
    EXPECT(isg_mask_nms_workspace(16, 1024, 1024) > 0);
    EXPECT(isg_mask_rle_workspace(16, 1024, 1024) > 0);
    {   // isg_mask_rle rejects these before any HIP call
        uint8_t px[16] = {};
        int64_t off[3] = {};
        uint32_t wk[64] = {};
        EXPECT(isg_mask_rle(px, 1, 65536, 32768, nullptr, nullptr, 1, nullptr, 0, off, wk,
                            nullptr) == ISG_ERR_INVALID);  // H*W == 2^31
        EXPECT(std::strstr(isg_last_error(), "2^31") != nullptr);
        EXPECT(isg_mask_rle(px, 1, 4, 4, nullptr, nullptr, 2, nullptr, 0, off, wk, nullptr) ==
               ISG_ERR_INVALID);  // max_sel > K with sel == NULL
        EXPECT(isg_mask_rle(px, 1, 4, 4, nullptr, nullptr, 1, nullptr, 8, off, wk, nullptr) ==
               ISG_ERR_INVALID);  // runs == NULL with runs_cap > 0
        EXPECT(isg_mask_rle(px, 1, 4, 4, nullptr, nullptr, 1, nullptr, 0, nullptr, wk, nullptr) ==
               ISG_ERR_INVALID);  // NULL offsets
    }
    EXPECT(isg_mask_rle_decode_workspace(16, 1024, 1024, 2049) == 8 * (2050 + 2));
    EXPECT(isg_mask_rle_decode_workspace(1, 65536, 32768, 16) == -1);
    EXPECT(isg_mask_rle_decode_workspace(1, 4, 4, -1) == -1);
    {   // isg_mask_rle_decode rejects these before any HIP call
        uint32_t rn[8] = {};
        int64_t off[4] = {}, tot[4] = {};
        uint64_t wk[16] = {};
        uint8_t px[64] = {};
        EXPECT(isg_mask_rle_decode(rn, 8, off, 0, 4, 4, nullptr, nullptr, nullptr, nullptr) ==
               ISG_OK);  // n == 0
        EXPECT(isg_mask_rle_decode(rn, 8, off, -1, 4, 4, px, tot, wk, nullptr) == ISG_ERR_INVALID);
        EXPECT(isg_mask_rle_decode(rn, 8, off, 1, 0, 4, px, tot, wk, nullptr) == ISG_ERR_INVALID);
        EXPECT(isg_mask_rle_decode(rn, 8, off, 1, 4, -4, px, tot, wk, nullptr) == ISG_ERR_INVALID);
        EXPECT(isg_mask_rle_decode(rn, -1, off, 1, 4, 4, px, tot, wk, nullptr) == ISG_ERR_INVALID);
        EXPECT(isg_mask_rle_decode(rn, 8, off, 1, 65536, 32768, px, tot, wk, nullptr) ==
               ISG_ERR_INVALID);  // H*W == 2^31
        EXPECT(std::strstr(isg_last_error(), "2^31") != nullptr);
        EXPECT(isg_mask_rle_decode(nullptr, 8, off, 1, 4, 4, px, tot, wk, nullptr) ==
               ISG_ERR_INVALID);  // runs == NULL with runs_cap > 0
        EXPECT(isg_mask_rle_decode(rn, 8, nullptr, 1, 4, 4, px, tot, wk, nullptr) == ISG_ERR_INVALID);
        EXPECT(isg_mask_rle_decode(rn, 8, off, 1, 4, 4, nullptr, tot, wk, nullptr) == ISG_ERR_INVALID);
        EXPECT(isg_mask_rle_decode(rn, 8, off, 1, 4, 4, px, nullptr, wk, nullptr) == ISG_ERR_INVALID);
        EXPECT(isg_mask_rle_decode(rn, 8, off, 1, 4, 4, px, tot, nullptr, nullptr) == ISG_ERR_INVALID);
        EXPECT(std::strstr(isg_last_error(), "NULL") != nullptr);
        EXPECT(isg_mask_rle_decode((const uint32_t*)((const char*)rn + 2), 4, off, 1, 4, 4, px, tot,
                                   wk, nullptr) == ISG_ERR_INVALID);  // runs not 4-B aligned
        EXPECT(isg_mask_rle_decode(rn, 8, (const int64_t*)((const char*)off + 4), 1, 4, 4, px, tot,
                                   wk, nullptr) == ISG_ERR_INVALID);  // offsets not 8-B aligned
        EXPECT(isg_mask_rle_decode(rn, 8, off, 1, 4, 4, px, (int64_t*)((char*)tot + 4), wk,
                                   nullptr) == ISG_ERR_INVALID);
        EXPECT(isg_mask_rle_decode(rn, 8, off, 1, 4, 4, px, tot, (char*)wk + 4, nullptr) ==
               ISG_ERR_INVALID);
        EXPECT(std::strstr(isg_last_error(), "alignment") != nullptr);
        EXPECT(isg_mask_rle_decode(rn, (int64_t)1 << 31, off, 1, 4, 4, px, tot, wk, nullptr) ==
               ISG_ERR_UNSUPPORTED);
    }

    EXPECT(isg_train_crop_workspace(8) == 8 * 2048 && isg_train_crop_workspace(0) == 0);
    {   // isg_train_crop rejects these before any HIP call (the descriptors are host memory)
        uint8_t px[4 * 6 * 5] = {};
        double kp[ISG_TRAIN_PARTS * 3] = {}, kpo[ISG_TRAIN_PARTS * 3] = {};
        int32_t wk[8] = {}, win[4] = {};
        float x[3 * 4] = {}, m[4] = {};
        isg_train_sample s{};
        s.img_off = 0; s.mask_off = 90; s.H = 6; s.W = 5; s.valid[2] = 5; s.valid[3] = 6;
        const int64_t nb = (int64_t)sizeof(px);
        EXPECT(isg_train_crop(px, nb, &s, kp, 0, 1, 2, wk, x, m, kpo, win, nullptr) == ISG_OK);  // n == 0
        EXPECT(isg_train_crop(nullptr, nb, &s, kp, 1, 1, 2, wk, x, m, kpo, win, nullptr) == ISG_ERR_INVALID);
        EXPECT(isg_train_crop(px, nb, nullptr, kp, 1, 1, 2, wk, x, m, kpo, win, nullptr) == ISG_ERR_INVALID);
        EXPECT(isg_train_crop(px, nb, &s, kp, 1, 1, 0, wk, x, m, kpo, win, nullptr) == ISG_ERR_INVALID);  // S
        EXPECT(isg_train_crop(px, nb, &s, kp, 2, 1, 2, wk, x, m, kpo, win, nullptr) == ISG_ERR_INVALID);  // n > B
        EXPECT(isg_train_crop(px, nb - 1, &s, kp, 1, 1, 2, wk, x, m, kpo, win, nullptr) == ISG_ERR_INVALID);
        EXPECT(std::strstr(isg_last_error(), "outside the arena") != nullptr);
        s.H = 0;
        EXPECT(isg_train_crop(px, nb, &s, kp, 1, 1, 2, wk, x, m, kpo, win, nullptr) == ISG_ERR_INVALID);
        s.H = 30000; s.W = 30000;
        EXPECT(isg_train_crop(px, nb, &s, kp, 1, 1, 2, wk, x, m, kpo, win, nullptr) == ISG_ERR_INVALID);
        EXPECT(std::strstr(isg_last_error(), "2^31") != nullptr);
    }
    {   // isg_train_crop_aug: the same checks, then every field of the host records
        uint8_t px[4 * 6 * 5] = {};
        double kp[ISG_TRAIN_PARTS * 3] = {}, kpo[ISG_TRAIN_PARTS * 3] = {};
        int32_t wk[8] = {}, win[4] = {};
        float x[3 * 4] = {}, m[4] = {};
        isg_train_sample s{};
        s.img_off = 0; s.mask_off = 90; s.H = 6; s.W = 5; s.valid[2] = 5; s.valid[3] = 6;
        isg_train_aug id{};
        id.rot_cos = 1.0; id.contrast = 1.f; id.mult[0] = id.mult[1] = id.mult[2] = 1.f;
        const int64_t nb = (int64_t)sizeof(px);
        auto call = [&](const isg_train_aug& a, int32_t n = 1, int32_t B = 1) {
            return isg_train_crop_aug(px, nb, &s, &a, 7, 0, kp, n, B, 2, wk, x, m, kpo, win, nullptr);
        };
        EXPECT(isg_record_size(21) == (int32_t)sizeof(isg_train_aug) && sizeof(isg_train_aug) == 64);
        EXPECT(call(id, 0) == ISG_OK);  // n == 0
        EXPECT(call(id, 2) == ISG_ERR_INVALID);  // n > B
        EXPECT(isg_train_crop_aug(px, nb, &s, nullptr, 7, 0, kp, 1, 1, 2, wk, x, m, kpo, win, nullptr) ==
               ISG_ERR_INVALID);
        EXPECT(isg_train_crop_aug(px, nb - 1, &s, &id, 7, 0, kp, 1, 1, 2, wk, x, m, kpo, win, nullptr) ==
               ISG_ERR_INVALID);
        EXPECT(std::strstr(isg_last_error(), "outside the arena") != nullptr);
        isg_train_aug a = id;
        a.jitter[3] = 1025;
        EXPECT(call(a) == ISG_ERR_INVALID && std::strstr(isg_last_error(), "jitter[3]") != nullptr);
        a = id; a.jitter[0] = -1025;
        EXPECT(call(a) == ISG_ERR_INVALID);
        a = id; a.rot_cos = 0.9; a.rot_sin = 0.5;
        EXPECT(call(a) == ISG_ERR_INVALID && std::strstr(isg_last_error(), "rotation") != nullptr);
        a = id; a.rot_sin = std::strtod("nan", nullptr);
        EXPECT(call(a) == ISG_ERR_INVALID);
        a = id; a.contrast = -1.f;
        EXPECT(call(a) == ISG_ERR_INVALID);
        a = id; a.noise = std::strtof("inf", nullptr);
        EXPECT(call(a) == ISG_ERR_INVALID);
        a = id; a.mult[2] = std::strtof("nan", nullptr);
        EXPECT(call(a) == ISG_ERR_INVALID && std::strstr(isg_last_error(), "mult") != nullptr);
        a = id; a.flip = 2;
        EXPECT(call(a) == ISG_ERR_INVALID);
    }

    // executor: a malformed record size, an unknown kind, then well-formed records whose
    // launches fail without a device (fix-ups and the side-stream batching run first)
    std::vector<char> blob;
    std::vector<char> big(9000, 0);
    char desc[64] = {};
    put_op(blob, 12, big.data(), (int)big.size(), {}, {});  // larger than the executor's buffer
    void* table[32] = {};
    EXPECT(isg_exec(blob.data(), 1, table, nullptr) == ISG_ERR_INVALID);
    blob.clear();
    put_op(blob, 77, desc, 16, {}, {});
    EXPECT(isg_exec(blob.data(), 1, table, nullptr) == ISG_ERR_INVALID);
    EXPECT(std::strstr(isg_last_error(), "unknown op kind") != nullptr);
    blob.clear();
    std::vector<char> arena(4096);
    table[0] = arena.data();
    struct { void* p; int64_t bytes; } ms{nullptr, 256};
    put_op(blob, 12, &ms, sizeof(ms), {isg_ref{0, 0, 128}}, {0});
    put_op(blob, 12, &ms, sizeof(ms), {isg_ref{0, 0, 0}}, {0}, /*side|fork_now*/ 1 | 4);
    const int rc = isg_exec_ms(blob.data(), 2, table, nullptr, nullptr);
    std::printf("exec of memset records without a device: rc %d (%s)\n", rc, isg_last_error());

    // host item arrays longer than one chunk
    std::vector<isg_bn> bns(3 * ISG_LIST_CHUNK + 5);
    for (auto& b : bns) { std::memset(&b, 0, sizeof(b)); b.C = 16; b.train = 1; b.count = 4.f; b.eps = 1e-5f; }
    const int rb = isg_bn_finalize(bns.data(), (int32_t)bns.size(), 0, nullptr);
    std::vector<isg_bn_update> ups(ISG_LIST_CHUNK + 1);
    std::memset(ups.data(), 0, ups.size() * sizeof(isg_bn_update));
    const int ru = isg_bn_update_running(ups.data(), (int32_t)ups.size(), nullptr);
    std::vector<isg_grad_final> gfs(2 * ISG_LIST_CHUNK);
    std::memset(gfs.data(), 0, gfs.size() * sizeof(isg_grad_final));
    const int rg = isg_grad_finalize(gfs.data(), (int32_t)gfs.size(), nullptr);
    std::printf("chunked item launches without a device: %d %d %d\n", rb, ru, rg);
    EXPECT(isg_bn_finalize(nullptr, 0, 0, nullptr) == ISG_OK || std::strlen(isg_last_error()) > 0);

    std::printf("%s: %d failure(s)\n", failures ? "FAIL" : "OK", failures);
    return failures ? 1 : 0;
}
