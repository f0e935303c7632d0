// Stand-alone host check of the latent samplers' layout derivation (csrc/sample_layout.hip: wan_lay / cog_lay / hy_lay, lay_derive, launch_limits) for a
// sanitizer build: every geometry of tests/test_gpu_wan_sampling.py, tests/test_gpu_cog_sampling.py and tests/test_gpu_hy_sampling.py must be accepted, every
// refused geometry of tests/test_wan_sampling_host.py, tests/test_cog_sampling_host.py and tests/test_hy_sampling_host.py refused with its code and text.
// Launches nothing and needs no GPU.
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I finetrainers_amd/csrc tools/sample_layout_hostcheck.hip -o tools/bin/sample_layout_hostcheck && tools/bin/sample_layout_hostcheck
#include <cstdio>
#include <cstring>
#include <string>

#include "../finetrainers_amd/csrc/sample_layout.hip"  // the derivation sits in the file's anonymous namespace

namespace ftmi {
static std::string g_last;
int set_error(int code, const char* msg) {
    g_last = msg;
    return code;
}
int check_launch(const char*) { return 0; }
}  // namespace ftmi

using namespace ftmi;

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            ++failures;                                                       \
            printf("line %d: %s (last error: %s)\n", __LINE__, #cond, g_last.c_str()); \
        }                                                                     \
    } while (0)

static ftmi_wan_sample_geometry wan(int B, int Cx, int F, int H, int W, int Kp, int copies, int P) {
    ftmi_wan_sample_geometry g = {};
    g.B = B; g.C = 16; g.Cx = Cx; g.F = F; g.H = H; g.W = W; g.pt = 1; g.ph = 2; g.pw = 2; g.Kp = Kp; g.copies = copies; g.P = P; g.po = 64;
    return g;
}
static ftmi_cog_sample_geometry cog(int B, int F, int H, int W, int pt, int P, int drop) {
    ftmi_cog_sample_geometry g = {};
    g.B = B; g.C = 16; g.F = F; g.H = H; g.W = W; g.p = 2; g.pt = pt; g.P = P; g.drop = drop;
    return g;
}
static ftmi_hy_sample_geometry hy(int B, int F, int H, int W, int pt, int P) {
    ftmi_hy_sample_geometry g = {};
    g.B = B; g.C = 16; g.F = F; g.H = H; g.W = W; g.p = 2; g.pt = pt; g.P = P;
    return g;
}

// an accepted layout: both launch limits hold, and the derived fields are the documented formulas
static void accepted(const Lay& l, long sc, long sf) {
    size_t lds_i = 0, lds_f = 0;
    EXPECT(launch_limits(l, true, "init", lds_i) == 0 && launch_limits(l, false, "finish", lds_f) == 0);
    EXPECT(l.pv == l.pt * l.ph * l.pw && l.Kc == l.C * l.pv && l.Kx == l.Cx * l.pv && l.ld == l.copies * l.Kp);
    EXPECT(l.S == (long)(l.F / l.pt) * (l.H / l.ph) * (l.W / l.pw) && l.seg_len == l.ph * l.W);
    EXPECT(l.pitch_f % 4 == 0 && l.pitch_f >= l.seg_len + 4 && l.pitch_h % 8 == 0 && l.pitch_h >= l.seg_len + 8);  // a run and the offset of its start inside a vector
    EXPECT(l.sc == sc && l.sf == sf);
    EXPECT(lds_i == (size_t)l.C * l.pt * l.pitch_f * 4 + (size_t)l.Cx * l.pt * l.pitch_h * 2 && lds_f == (size_t)l.C * l.pt * l.pitch_h * 2);
}

int main() {
    Lay l;
    size_t lds0 = 0;
    // ---- accepted: the GPU tests' geometries
    const int wan_layouts[3][3] = {{64, 0, 1}, {192, 20, 1}, {128, 16, 2}};  // (Kp, Cx, copies): t2v, i2v, control
    const int wan_grids[4][3] = {{1, 2, 2}, {3, 4, 6}, {2, 4, 8}, {2, 8, 12}};
    for (auto& lay : wan_layouts)
        for (auto& gr : wan_grids)
            for (int B = 1; B <= 2; ++B)
                for (int P = 1; P <= 2; ++P) {
                    EXPECT(wan_lay(wan(B, lay[1], gr[0], gr[1], gr[2], lay[0], lay[2], P), "wan", l) == 0);
                    EXPECT(l.drop == 0 && l.Kp == lay[0] && l.P == P);
                    accepted(l, (long)gr[0] * gr[1] * gr[2], (long)gr[1] * gr[2]);
                }
    const int cog_grids[7][5] = {{1, 2, 2, 1, 0}, {3, 4, 6, 1, 0}, {2, 4, 8, 1, 0}, {2, 4, 8, 2, 0}, {2, 4, 8, 2, 1}, {4, 4, 6, 2, 1}, {3, 8, 12, 1, 0}};
    for (auto& gr : cog_grids)
        for (int B = 1; B <= 2; ++B)
            for (int P = 1; P <= 2; ++P) {
                EXPECT(cog_lay(cog(B, gr[0], gr[1], gr[2], gr[3], P, gr[4]), "cog", l) == 0);
                EXPECT(l.Cx == 0 && l.copies == 1 && l.Kp == l.Kc && l.ld == l.Kc && l.drop == gr[4] && l.ph == 2 && l.pw == 2);
                accepted(l, (long)gr[1] * gr[2], 16L * gr[1] * gr[2]);
            }
    // ---- refused: the host tests' geometries (base: B 1, C 16, F 2, H 8, W 12, patch (1, 2, 2), Kp 64, one copy, P 2)
    auto wbad = [&](ftmi_wan_sample_geometry g, int code, const char* text) {
        EXPECT(wan_lay(g, "wan_sample_step", l) == code && g_last.find(text) != std::string::npos && g_last.rfind("wan_sample_step: ", 0) == 0);
    };
    ftmi_wan_sample_geometry w = wan(1, 0, 2, 8, 12, 64, 1, 2), g = w;
    g = w; g.C = 15; g.po = 60; wbad(g, FTMI_ERR_UNSUPPORTED, "multiples of 8");
    g = w; g.Kp = 68; wbad(g, FTMI_ERR_UNSUPPORTED, "row stride");
    g = w; g.po = 128; wbad(g, FTMI_ERR_INVALID, "must equal po");
    g = w; g.po = 32; wbad(g, FTMI_ERR_INVALID, "must equal po");
    g = w; g.W = 13; wbad(g, FTMI_ERR_UNSUPPORTED, "whole patches");
    g = w; g.H = 7; wbad(g, FTMI_ERR_UNSUPPORTED, "whole patches");
    g = w; g.pt = 2; g.F = 3; wbad(g, FTMI_ERR_UNSUPPORTED, "whole patches");
    g = w; g.Cx = 20; wbad(g, FTMI_ERR_INVALID, "do not fit");
    g = w; g.copies = 3; wbad(g, FTMI_ERR_INVALID, "copies");
    g = w; g.P = 3; wbad(g, FTMI_ERR_INVALID, "P is 2");
    g = w; g.C = 24; g.po = 96; g.Kp = 128; wbad(g, FTMI_ERR_UNSUPPORTED, "divide 2048");
    g = w; g.B = 0; wbad(g, FTMI_ERR_INVALID, "positive");
    g = w; g.Cx = 20; g.Kp = 192; EXPECT(wan_lay(g, "wan", l) == 0);  // accepted here: wan_sample_init refuses it for the missing tensor
    auto cbad = [&](ftmi_cog_sample_geometry g, int code, const char* text) {
        EXPECT(cog_lay(g, "cog_sample_step", l) == code && g_last.find(text) != std::string::npos && g_last.rfind("cog_sample_step: ", 0) == 0);
    };
    ftmi_cog_sample_geometry c0 = cog(1, 2, 8, 12, 1, 2, 0), c = c0;
    c = c0; c.C = 15; cbad(c, FTMI_ERR_UNSUPPORTED, "multiple of 8");
    c = c0; c.C = 8; EXPECT(cog_lay(c, "cog", l) == 0);  // the layout holds; cog_sample refuses the model width
    c = c0; c.W = 13; cbad(c, FTMI_ERR_UNSUPPORTED, "whole patches");
    c = c0; c.H = 7; cbad(c, FTMI_ERR_UNSUPPORTED, "whole patches");
    c = c0; c.pt = 2; c.F = 3; cbad(c, FTMI_ERR_UNSUPPORTED, "whole patches");
    c = c0; c.pt = 3; c.F = 3; cbad(c, FTMI_ERR_UNSUPPORTED, "patch_size_t is 1 or 2");
    c = c0; c.P = 3; cbad(c, FTMI_ERR_INVALID, "P is 2");
    c = c0; c.drop = 1; cbad(c, FTMI_ERR_INVALID, "drop");
    c = c0; c.pt = 2; c.drop = 2; cbad(c, FTMI_ERR_INVALID, "drop");
    c = c0; c.B = 0; cbad(c, FTMI_ERR_INVALID, "positive");
    // ---- HunyuanVideo: CogVideoX's layout over [B, C, F, H, W] latents (Wan's strides), nothing dropped
    const int hy_grids[4][3] = {{1, 2, 2}, {3, 4, 6}, {2, 4, 8}, {3, 8, 12}};
    for (auto& gr : hy_grids)
        for (int B = 1; B <= 2; ++B)
            for (int P = 1; P <= 2; ++P) {
                EXPECT(hy_lay(hy(B, gr[0], gr[1], gr[2], 1, P), "hy", l) == 0);
                EXPECT(l.Cx == 0 && l.copies == 1 && l.Kp == l.Kc && l.ld == l.Kc && l.Kc == 64 && l.drop == 0 && l.ph == 2 && l.pw == 2 && l.P == P);
                accepted(l, (long)gr[0] * gr[1] * gr[2], (long)gr[1] * gr[2]);
            }
    auto hbad = [&](ftmi_hy_sample_geometry g, int code, const char* text) {
        EXPECT(hy_lay(g, "hy_sample_step", l) == code && g_last.find(text) != std::string::npos && g_last.rfind("hy_sample_step: ", 0) == 0);
    };
    ftmi_hy_sample_geometry h0 = hy(1, 3, 8, 12, 1, 1), h = h0;
    h = h0; h.C = 15; hbad(h, FTMI_ERR_UNSUPPORTED, "multiple of 8");
    h = h0; h.C = 8; EXPECT(hy_lay(h, "hy", l) == 0);  // the layout holds; hy_sample refuses the patch width
    h = h0; h.W = 13; hbad(h, FTMI_ERR_UNSUPPORTED, "whole patches");
    h = h0; h.H = 7; hbad(h, FTMI_ERR_UNSUPPORTED, "whole patches");
    h = h0; h.pt = 2; hbad(h, FTMI_ERR_UNSUPPORTED, "whole patches");
    h = h0; h.P = 3; hbad(h, FTMI_ERR_INVALID, "P is 2");
    h = h0; h.P = 0; hbad(h, FTMI_ERR_INVALID, "P is 2");
    h = h0; h.B = 0; hbad(h, FTMI_ERR_INVALID, "positive");
    h = h0; h.p = 0; hbad(h, FTMI_ERR_INVALID, "positive");
    EXPECT(hy_lay(hy(1, 1, 2, 8194, 1, 1), "hy", l) == FTMI_ERR_UNSUPPORTED && g_last.find("patch or row too wide") != std::string::npos);
    EXPECT(hy_lay(hy(0x7fffffff, 1, 2, 2, 1, 2), "hy", l) == 0 && launch_limits(l, true, "hy", lds0) == 0 && launch_limits(l, false, "hy", lds0) == 0);
    EXPECT(hy_lay(hy(0x7fffffff, 2, 2, 2, 1, 2), "hy_sample_init", l) == FTMI_ERR_UNSUPPORTED && g_last == "hy_sample_init: too many elements for one launch");
    // ---- the launch limits: the LDS, whole 16-byte vectors, the grids
    size_t lds = 0;
    EXPECT(cog_lay(cog(1, 1, 2, 8192, 1, 1, 0), "cog", l) == 0 && launch_limits(l, true, "cog_sample_init", lds) == FTMI_ERR_UNSUPPORTED &&
           g_last == "cog_sample_init: a row of patches does not fit the LDS");
    EXPECT(cog_lay(cog(1, 1, 2, 8194, 1, 1, 0), "cog", l) == FTMI_ERR_UNSUPPORTED && g_last.find("patch or row too wide") != std::string::npos);
    // (B C F H W = B S Kc and Kc % 8 == 0, so an accepted layout's tensors are always whole vectors: that refusal has no geometry to show it)
    // the largest accepted sizes stay inside long arithmetic (UBSan watches the products); one workgroup more is refused by the grid bound
    EXPECT(cog_lay(cog(1, 2, 2, 8192, 2, 2, 1), "cog", l) == 0 && l.Kc == 128 && l.S == 4096);
    EXPECT(cog_lay(cog(0x7fffffff, 1, 2, 2, 1, 2, 0), "cog", l) == 0 && launch_limits(l, true, "cog", lds) == 0 && launch_limits(l, false, "cog", lds) == 0);
    EXPECT(cog_lay(cog(0x7fffffff, 2, 2, 2, 1, 2, 0), "cog_sample_init", l) == FTMI_ERR_UNSUPPORTED && g_last == "cog_sample_init: too many elements for one launch");
    g = wan(0x7fffffff, 0, 1, 2, 2, 65536, 2, 2);
    EXPECT(wan_lay(g, "wan_sample_init", l) == FTMI_ERR_UNSUPPORTED && g_last == "wan_sample_init: too many elements for one launch");
    g = wan(0x7fffffff, 20, 1, 2, 2, 192, 1, 2);
    EXPECT(wan_lay(g, "wan", l) == 0 && launch_limits(l, true, "wan", lds) == 0);
    printf("sample_layout_hostcheck: %d failure(s)\n", failures);
    return failures != 0;
}
