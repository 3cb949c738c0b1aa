"""Records tests/golden/conv_launch_shapes.json: which kernel, tile, grid, split-K factor, epilogue width and GroupNorm
chunk count the fp32 conv launcher chose for a table of shapes BEFORE that choice became one function (conv_shape,
csrc/kernels_conv.hip).  Runs on the CPU in seconds; needs git and a host C++ compiler.

    python tests/golden/make_conv_launch_shapes.py [--rev COMMIT] [--cxx g++] [OUT]

The committed file was recorded with --rev at its default: the last commit whose launch_conv_igemm decided the launch
itself, on every launch, from the raw pointers and a process-wide CU count.  Recording it from a later commit is not
possible (the code this recipe cuts out is gone) and recording it from conv_shape would pin that function to itself.

Recipe.  From `git show REV:kidney-diffusion_amd/csrc/kernels_conv.hip` the decision code is cut out unchanged - everything
from conv_macs() to the end of launch_conv_igemm(): fast_shape_ok, conv_ksplit, conv_seg_chunks, launch_conv_fast,
conv_wide_ok - and ConvParams with its enums from that commit's common.h.  Two textual changes: hipLaunchKernelGGL becomes
a recorder of the kernel's name with its template arguments, the grid, the block and the ConvParams it was handed (ksplit
and wide_epilogue are read from there), and the `static int cus` with its device query becomes a value the driver sets.
The copy is compiled for the host with a small main() and fed the table.  Pointers are made up from the alignment flags
the way that commit's plan builder probed its own launcher: 4096 k for a 16-byte aligned address, 4 more for one that is
not, null for an absent map.  conv_seg_chunks is asked as the plan builder asked it.  The driver also launches every
case a second time with seg_partial set where the chunk count is positive, and requires the same record: for a launch
that code accepts, the choice does not depend on whether the partials are wanted.

The table (build_cases): every row of test_kernels_gpu.test_conv_igemm as kd_conv2d_nhwc fills it; the batched position
GEMMs of the Winograd layers (wz_rows, 16 and 36 positions) at two CU counts; a synthetic grid over M, Cin, Cout and the
window at 256 and 120 CUs that crosses every threshold of that code on both sides; and variations of the output mode, the
added maps, the statistics offset and each alignment flag.  check_coverage() requires that the recorded choices contain
every kernel / tile variant, split and unsplit launches, both epilogue widths and launches with and without partials.
The JSON holds results only, in the table's order, and a digest of the table; tests/test_conv_shapes.py rebuilds the table
with build_cases().
"""
import argparse
import hashlib
import itertools
import json
import re
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
PARENT = "cc610a8"   # "Fused-tile stage driver in named parts; one path for 1 or N shards"

# the ints of a case, in the order kd_conv_launch_shape takes them (include/kd_engine.h)
GEOM = ["B", "Hi", "Wi", "Cin", "ldx", "Ho", "Wo", "Cout", "KH", "KW", "stride", "pad", "rr_cin", "act", "ldres", "ldgs",
        "out_mode", "ldy", "yoff", "wz_rows", "wz_count", "seg_c0"]
Y, BIAS, RES, GATE_SRC, GATE, PARTIAL = 1, 2, 4, 8, 16, 32   # bits of `has` and `al16`
ALL = Y | BIAS | RES | GATE_SRC | GATE | PARTIAL
SHAPE = ["igemm", "bm", "bn", "waves_m", "waves_n", "grid_x", "grid_y", "grid_z", "block", "ksplit", "wide", "seg_chunks"]
NHWC, PIXSHUF, NCHW = 0, 1, 2


def geom(B, Hi, Wi, Cin, Cout, K=1, stride=1, pad=0, **kw):
    g = dict.fromkeys(GEOM, 0)
    g.update(B=B, Hi=Hi, Wi=Wi, Cin=Cin, ldx=Cin, Cout=Cout, KH=K, KW=K, stride=stride, pad=pad,
             Ho=(Hi + 2 * pad - K) // stride + 1, Wo=(Wi + 2 * pad - K) // stride + 1, out_mode=NHWC, ldy=Cout)
    g.update(kw)
    return g


def conv2d_entry(B, H, W, Cin, Cout, K, stride, pad, act):
    """ConvParams as kd_conv2d_nhwc (csrc/api.inc) fills it for a row of test_conv_igemm."""
    g = geom(B, H, W, Cin, Cout, K, stride, pad, act=act & 0xff)
    if act & 0x100:
        g.update(KW=1, Cin=K * Cin, rr_cin=Cin)
    if act & 0x200:
        g.update(out_mode=PIXSHUF, ldy=Cout // 4)
    return g


def conv_igemm_rows():
    sys.path[:0] = [str(REPO / "tests"), str(REPO)]
    import test_kernels_gpu
    mark = [m for m in test_kernels_gpu.test_conv_igemm.pytestmark if m.name == "parametrize"][0]
    return [tuple(r) for r in mark.args[1]]


def build_cases():
    cases = []   # (group, geometry, has, al16, cus)

    def add(group, g, has=Y | BIAS | PARTIAL, al16=ALL, cus=256):
        cases.append((group, g, has, al16 & has, cus))

    for row in conv_igemm_rows():
        add("conv_igemm", conv2d_entry(*row))
    # the batched position GEMMs (kd_conv3x3_winograd_nhwc / kd_conv3x3_winograd4_nhwc, Builder::wino*): no bias, no scratch
    for cus, npos, Mt, Cin, Cout in itertools.product((256, 120), (16, 36), (128, 256, 384, 1024, 2304), (128,), (64, 128, 1024)):
        add("positions", geom(1, 1, npos * Mt, Cin, Cout, wz_rows=Mt, wz_count=npos), has=Y, cus=cus)
    # the grid: M <= 64 | > 64; tiles256 = ceil(M / 256) ceil(Cout / 128) around 512 (65536 x 256 | 65280 x 256) and the
    # 128 x 128 count around 512 (16384 x 512 | 16256 x 512); k-chunks 8 | 9 and 63 | 64 (1x1), 9 x Cin / 32 (3x3); Cout
    # 32 | 36, 64 | 68; split-K: 128 x 64 tiles around 256 (1024 x 1984 | 2048), k-chunks 15 | 16; Cin % 32 != 0 (36)
    # (two products, the small maps and the large ones, so that the table stays a few hundred cases)
    small = itertools.product((64, 65, 1024), (36, 256, 480, 512, 2048), (32, 36, 64, 68, 256, 1984, 2048))
    large = itertools.product((16256, 16384, 65280, 65536), (256, 288, 2016, 2048), (64, 256, 512))
    for cus, (M, Cin, Cout), K in itertools.product((256, 120), list(small) + list(large), (1, 3)):
        add("grid", geom(1, 1, M, Cin, Cout, K, 1, K // 2), cus=cus)
    # images: Ho Wo % 32 (48 | 64 pixels per image), maps whose 3x3 form passes the 2^31-byte span of the fast kernel
    for hw, Cout in itertools.product((48, 64), (64, 128)):
        add("images", geom(4, 1, hw, 64, Cout))
        add("images", geom(4, 1, hw, 512, Cout, 3, 1, 1))
    add("images", geom(1, 512, 512, 2048, 128, 3, 1, 1))
    add("images", geom(1, 512, 512, 2048, 128))
    # output modes, added maps, statistics offsets and every alignment flag, over shapes that take each family of kernel:
    # fast 128 x 64, fast 256 x 128, generic, split-K at M = 64 and at M = 256
    bases = [geom(2, 16, 16, 64, 128), geom(8, 128, 128, 32, 128, 3, 1, 1), geom(2, 16, 16, 36, 48, 3, 1, 1),
             geom(1, 8, 8, 1024, 1024, 3, 1, 1), geom(1, 16, 16, 512, 320)]
    for b in bases:
        for mode in (NHWC, PIXSHUF, NCHW):
            for maps in (0, RES, GATE_SRC | GATE, RES | GATE_SRC | GATE) if mode != NCHW else (0, RES | GATE_SRC | GATE):
                g = dict(b, out_mode=mode, ldy={NHWC: b["Cout"], PIXSHUF: b["Cout"] // 4, NCHW: 0}[mode],
                         ldres=b["Cout"] if maps & RES else 0, ldgs=b["Cout"] if maps & GATE_SRC else 0)
                has = Y | BIAS | PARTIAL | maps
                add("epilogue", g, has)
                for bit in (Y, BIAS, RES, GATE_SRC, GATE):   # (an unaligned split-K scratch is refused)
                    if has & bit:
                        add("epilogue", g, has, ALL & ~bit)
                add("epilogue", g, has & ~PARTIAL)   # no scratch: never split
                add("epilogue", g, has & ~BIAS)
        # strided rows, a channel slice of a wider map, a statistics segment that starts off a 16-channel boundary
        for ldy, yoff, seg_c0, ldres, act in ((b["Cout"] + 64, 64, 64, b["Cout"] + 32, 0), (b["Cout"] + 64, 32, 16, b["Cout"], 0),
                                              (b["Cout"] + 64, 24, 8, b["Cout"], 0), (b["Cout"] + 64, 24, 0, b["Cout"], 0),
                                              (b["Cout"] + 6, 2, 2, b["Cout"] + 2, 0), (b["Cout"], 0, 0, b["Cout"], 1)):
            add("epilogue", dict(b, ldy=ldy, yoff=yoff, seg_c0=seg_c0, ldres=ldres, act=act), Y | BIAS | PARTIAL | RES)
            add("epilogue", dict(b, ldy=ldy, yoff=yoff, seg_c0=seg_c0, ldgs=ldres, act=act), Y | BIAS | PARTIAL | GATE_SRC | GATE)
    # PixelShuffle statistics: Cout / 4 % 32 and Wo % 32
    for W, Cout in itertools.product((16, 32), (128, 256)):
        add("epilogue", geom(2, 32, W, 64, Cout, out_mode=PIXSHUF, ldy=Cout // 4))
    return cases


def case_row(case):
    """The ints kd_conv_launch_shape takes for a case of build_cases(): the geometry in GEOM's order, has, al16, cus."""
    _, g, has, al, cus = case
    return [g[k] for k in GEOM] + [has, al, cus]


def cases_digest(cases):
    return hashlib.sha256(json.dumps([[c[0]] + case_row(c) for c in cases]).encode()).hexdigest()


PRELUDE = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
typedef void* hipStream_t;
struct dim3 { unsigned x, y, z; dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {} };
constexpr int kd_switch(const char*, int dflt) { return dflt; }
static std::string g_error;
#define KD_REQUIRE(cond, msg) do { if (!(cond)) { g_error = #cond; return 1; } } while (0)
#define KD_HIP_CHECK(expr) do { (void)(expr); } while (0)
static int hipGetLastError() { return 0; }
constexpr int BK = 32;
static int g_cus = 0;
struct Launch { std::string kernel; dim3 grid, block; int ksplit, wide; };
static Launch g_first;
static int g_launches = 0;
"""

RECORDER = r"""
static void record(const char* kernel, dim3 grid, dim3 block, const ConvParams& q) {
  if (g_launches++ == 0) g_first = Launch{kernel, grid, block, q.ksplit, q.wide_epilogue};
}
static void record(const char* kernel, dim3 grid, dim3 block, const ConvParams& q, int64_t) { record(kernel, grid, block, q); }
#define hipLaunchKernelGGL(k, grid, block, lds, s, ...) record(#k, grid, block, __VA_ARGS__)
"""

MAIN = r"""
}  // namespace kd
using namespace kd;
static void* fake(unsigned has, unsigned al, unsigned bit, int k) {
  return (has & bit) ? (void*)(uintptr_t)(4096 * k + ((al & bit) ? 0 : 4)) : nullptr;
}
int main() {
  int v[%(NG)d];
  unsigned has, al;
  for (;;) {
    for (int i = 0; i < %(NG)d; ++i)
      if (scanf("%%d", &v[i]) != 1) return 0;
    if (scanf("%%u %%u %%d", &has, &al, &g_cus) != 3) return 1;
    ConvParams p{};
    int i = 0;
%(FILL)s
    p.x = (const float*)fake(1, 1, 1, 1);
    p.w = (const float*)fake(1, 1, 1, 2);
    p.y = (float*)fake(has, al, 1, 3);
    p.bias = (const float*)fake(has, al, 2, 4);
    p.res = (const float*)fake(has, al, 4, 5);
    p.gate_src = (const float*)fake(has, al, 8, 6);
    p.gate = (const float*)fake(has, al, 16, 7);
    p.partial = (float*)fake(has, al, 32, 8);
    const int chunks = conv_seg_chunks(p);
    Launch rec[2];
    int rc[2];
    for (int pass = 0; pass < 2; ++pass) {   // without and (where the launch can leave them) with the GroupNorm partials
      ConvParams q = p;
      if (pass == 1 && chunks > 0) {
        q.seg_partial = (double*)fake(1, 1, 1, 9);
        q.seg_nseg = 1;
      }
      g_launches = 0;
      g_error.clear();
      rc[pass] = launch_conv_igemm(q, nullptr);
      rec[pass] = g_first;
    }
    const Launch &a = rec[0], &b = rec[1];
    // (a launch refused only with the partials - split-K wants an aligned output for them - chose nothing else)
    if ((rc[1] && !rc[0] && g_error.find("seg_partial") == std::string::npos) || (rc[0] && !rc[1]) ||
        (!rc[0] && !rc[1] && (a.kernel != b.kernel || a.grid.x != b.grid.x || a.grid.y != b.grid.y || a.grid.z != b.grid.z ||
                                     a.ksplit != b.ksplit || a.wide != b.wide))) {
      printf("MISMATCH with seg_partial set\n");
      return 2;
    }
    if (rc[0]) printf("refused %%s\n", g_error.c_str());
    else printf("%%s | %%u %%u %%u %%u %%d %%d %%d\n", a.kernel.c_str(), a.grid.x, a.grid.y, a.grid.z, a.block.x,
                a.ksplit > 1 ? a.ksplit : 1 /* (unsplit launches left the field at 0; the kernels ask ksplit > 1) */, a.wide, chunks);
  }
}
"""


def git_show(rev, path):
    return subprocess.run(["git", "-C", str(REPO), "show", f"{rev}:{path}"], check=True, capture_output=True, text=True).stdout


def recorder_source(rev):
    conv = git_show(rev, "kidney-diffusion_amd/csrc/kernels_conv.hip")
    common = git_show(rev, "kidney-diffusion_amd/csrc/common.h")
    enums = re.search(r"enum Act \{.*?\};\s*enum OutMode \{.*?\};", common, re.S).group(0)
    params = re.search(r"struct ConvParams \{.*?\n\};", common, re.S).group(0)
    start = conv.index("int64_t conv_macs(const ConvParams& p) {")
    end = conv.index("// ------------------------------------------------------------------------------ weight packing")
    code = conv[start:end]
    code, n = re.subn(r"static int cus = 0;\s*if \(!cus\) \{.*?\n    \}\n", "const int cus = g_cus;\n", code, flags=re.S)
    assert n == 1 and "hipGetDeviceProperties" not in code and code.count("hipLaunchKernelGGL") == 16, (n, code.count("hipLaunchKernelGGL"))
    fill = "\n".join(f"    p.{name} = v[i++];" for name in GEOM)
    return (PRELUDE + "namespace kd {\n" + enums + "\n" + params + "\n" + RECORDER + code + MAIN % {"NG": len(GEOM), "FILL": fill})


def record(cases, rev, cxx):
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = Path(tmp) / "conv_launch_recorder.cpp", Path(tmp) / "conv_launch_recorder"
        src.write_text(recorder_source(rev))
        subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-o", str(exe), str(src)], check=True)
        feed = "".join(" ".join(map(str, case_row(c))) + "\n" for c in cases)
        out = subprocess.run([str(exe)], input=feed, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(cases), (len(out), len(cases))
    shapes = []
    for line in out:
        if line.startswith("refused"):
            shapes.append(None)
            continue
        kernel, nums = line.split(" | ")
        m = re.fullmatch(r"\(conv_(buf|igemm)_kernel<(\d+), (\d+), (\d+), (\d+)(?:, \d+)?>\)", kernel)
        assert m, kernel
        shapes.append([int(m.group(1) == "igemm")] + [int(x) for x in m.groups()[1:]] + [int(x) for x in nums.split()])
    return shapes


def check_coverage(shapes):
    """What the issue of the refactor asks of the golden: the code of before alone reaches all of it over this table."""
    ok = [dict(zip(SHAPE, s)) for s in shapes if s is not None]
    variants = {(s["igemm"], s["bm"], s["bn"]) for s in ok}
    want = {(0, 256, 128), (0, 128, 128), (0, 128, 64), (0, 64, 128), (1, 128, 32), (1, 128, 64), (1, 64, 128), (1, 128, 128)}
    assert variants == want, sorted(want - variants)
    assert {s["ksplit"] > 1 for s in ok} == {False, True}
    assert {s["wide"] for s in ok} == {0, 1}
    assert {s["seg_chunks"] > 0 for s in ok} == {False, True}
    return variants


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default=PARENT)
    ap.add_argument("--cxx", default="g++")
    ap.add_argument("out", nargs="?", default=str(HERE / "conv_launch_shapes.json"))
    a = ap.parse_args()
    cases = build_cases()
    shapes = record(cases, a.rev, a.cxx)
    check_coverage(shapes)
    assert all(sh is not None for sh in shapes), "that code refused a case of the table: a refused launch pins nothing"
    groups = {}
    for c in cases:
        groups[c[0]] = groups.get(c[0], 0) + 1
    # results only, in the order of build_cases(): the test rebuilds the table with this module and holds it to the digest
    head = {"recorded_from": a.rev, "shape_fields": SHAPE, "cases_sha256": cases_digest(cases), "groups": groups}
    rows = [", ".join(json.dumps(sh) for sh in shapes[i:i + 12]) for i in range(0, len(shapes), 12)]
    Path(a.out).write_text("{\n" + ",\n".join(f' "{k}": {json.dumps(v)}' for k, v in head.items()) + ',\n "shapes": [\n  '
                           + ",\n  ".join(rows) + "\n ]\n}\n")
    print(f"{len(shapes)} shapes {groups}, variants {sorted(check_coverage(shapes))} -> {a.out}")


if __name__ == "__main__":
    main()
