"""conv4.hip's chooser (csrc/conv4_forms.h: choose_v4, the list of instantiated forms, the name printer), compiled for the host and asked
every question the engine can ask it; the answers are held to tests/golden/v4_forms.json.

The golden was recorded from the commit BEFORE the chooser moved into conv4_forms.h (316389b), not from the code under test.  Recipe: a
scratch unit that #includes that commit's conv4.hip -- with the body of launch_v4_k replaced by one that prints its fourteen template
arguments into a buffer instead of launching -- and exports v4f_query as below (supported = conv_v4_supports, name = conv_v4_variant,
geometry = choose_v4's, block threads = 64 nw max(duo, 1)); every pointer choose_v4 tests is a non-null dummy, it inspects no memory.
Built twice (product, -DSS_DEVBUILD), loaded with ctypes on a machine without a GPU, driven by queries() / DEV_ENVS of this file, one
child process per environment, and written out by pack().  For every supported query launch_conv3x3_v4 succeeded there, with the
chooser's geometry, and the instantiation it reached was the one conv_v4_variant printed: the golden holds no corrected name.
"""
import ctypes
import hashlib
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "v4_forms.json")

# build_model's table (csrc/weights.hip): name, H, W, C0, C1, Cout, the block pools
LAYERS = [("conv1_1", 128, 256, 1, 0, 32, True), ("conv2_1", 64, 128, 32, 0, 64, True), ("conv3_1", 32, 64, 64, 0, 96, True),
          ("conv4_1", 16, 32, 96, 0, 128, True), ("conv_bottleneck", 8, 16, 128, 0, 128, False), ("encoder_out", 8, 16, 128, 0, 128, False),
          ("conv6", 16, 32, 128, 128, 96, False), ("conv7", 32, 64, 96, 96, 64, False), ("conv8", 64, 128, 64, 64, 32, False),
          ("conv9_1", 128, 256, 32, 32, 32, False), ("spec_output_conv.0", 128, 256, 32, 0, 32, False)]
RES_OUT, PLAIN, RES_IN, POOL, PROJ, FIRST, RANK1, FLAT = 1, 2, 4, 8, 16, 32, 64, 128
DEV_ENVS = ["", "SOFTSPOKEN_PF2=0", "SOFTSPOKEN_DUO=0", "SOFTSPOKEN_DUO=2", "SOFTSPOKEN_DUO_H8=0", "SOFTSPOKEN_RING=0", "SOFTSPOKEN_RING=2",
            "SOFTSPOKEN_RPROJ=0", "SOFTSPOKEN_RPROJ=1", "SOFTSPOKEN_GRES=0", "SOFTSPOKEN_BPC=1"]
FORM_FIELDS = ["NT", "NW", "BRES", "RES", "RADD", "POOL", "RP", "FIRST", "FLAT", "PF2", "SPLIT", "RANK1", "NH", "GRES"]
N_OUT = 8 + len(FORM_FIELDS) + 1


def _kinds(layer):
    """(flags, C0, C1, C0x, C1x, store_out) of the launches a block can ask for: A's 3x3 input is the block input, B's is h."""
    name, _, _, c0, c1, co, pools = layer
    pool = [0, POOL] if pools else [0]                   # (a pooling block's B launch: also asked without the pooled output)
    kinds = [(RES_OUT, c0, c1, 0, 0, 1), (PLAIN, c0, c1, 0, 0, 1)]
    kinds += [(RES_IN | p, co, 0, 0, 0, 1) for p in pool]
    kinds += [(PROJ | p, co, 0, c0, c1, 1) for p in pool]
    if name == "conv1_1":                                # FIRST (bf16), RANK1 with and without the first conv (f16x2)
        kinds += [(FIRST | RANK1 | POOL, co, 0, 0, 0, 1), (RANK1 | POOL, co, 0, 0, 0, 1)]
    if name == "conv9_1":                                # FLAT, with the r tensor and with the projection in B
        kinds += [(FLAT | RES_IN, co, 0, 0, 0, so) for so in (0, 1)] + [(FLAT | PROJ, co, 0, c0, c1, so) for so in (0, 1)]
    return kinds


def queries(ns=(1, 1005), cus=(256, 8)):
    """Rows of (prec, NT, num_cus, N, H, W, C0, C1, Cout, flags, C0x, C1x, store_out)."""
    qs = []
    for prec in (1, 2):
        for layer in LAYERS:
            _, H, W, _, _, co, _ = layer
            for flags, c0, c1, c0x, c1x, so in _kinds(layer):
                for nt in (1, 2, 3):
                    if co % (32 * nt):
                        continue
                    for n in ns:
                        for cu in cus:
                            qs.append((prec, nt, cu, n, H, W, c0, c1, co, flags, c0x, c1x, so))
    return qs


def dev_queries():
    return queries(ns=(1005,), cus=(256,))


def digest(qs):
    return hashlib.sha1(json.dumps(qs).encode()).hexdigest()


def ask(lib_path, qs):
    """Answers of the library at lib_path: None (not supported) or (name, grid, block threads, LDS bytes, total, lds_b, tiles_y, tiles_x),
    and the rest of v4f_query's output row."""
    L = ctypes.CDLL(lib_path)
    out = (ctypes.c_int * N_OUT)()
    name, launched = ctypes.create_string_buffer(256), ctypes.create_string_buffer(256)
    ans, extra = [], []
    for q in qs:
        L.v4f_query((ctypes.c_int * len(q))(*q), out, name, launched)
        ans.append((name.value.decode(),) + tuple(out[1:8]) if out[0] else None)
        extra.append((name.value.decode(), launched.value.decode(), tuple(out[8:])))
    return ans, extra


def pack(product, dev):
    """The golden file's content: names and answer rows interned, per query an index into the rows (-1: not supported)."""
    names, rows = [], []

    def idx(ans):
        o = []
        for a in ans:
            if a is None:
                o.append(-1)
                continue
            if a[0] not in names:
                names.append(a[0])
            r = [names.index(a[0])] + list(a[1:])
            if r not in rows:
                rows.append(r)
            o.append(rows.index(r))
        return o

    g = {"product": idx(product), "dev": {e: idx(a) for e, a in dev.items()}}
    g.update(names=names, rows=rows, product_queries=digest(queries()), dev_queries=digest(dev_queries()),
             columns=["name", "grid", "block", "lds", "total", "lds_b", "tiles_y", "tiles_x"])
    return g


def unpack(g, key, env=None):
    ix = g[key] if env is None else g[key][env]
    return [None if i < 0 else (g["names"][g["rows"][i][0]],) + tuple(g["rows"][i][1:]) for i in ix]


# The unit under test: the host-only header, no kernel in it.  launch_conv3x3_v4 (conv4.hip) does exactly what v4f_query does up to the
# lookup -- choose_v4, then v4_form_index(c.form) into the table the same list expands to -- and conv_v4_variant prints v4_form_name of
# that same c.form: the name in the stats and the instantiation launched come from one V4Form object by construction.
_SRC = r"""
#include "conv4_forms.h"
#include <cstring>
extern "C" {
// q: prec, NT, num_cus, N, H, W, C0, C1, Cout, flags, C0x, C1x, store_out
// out: ok, grid, block, lds, total, lds_b, tiles_y, tiles_x, the form's fourteen fields, its index in the list (-1: not in it)
int v4f_query(const int* q, int* out, char* name, char* launched) {
    using namespace ss;
    void* const P = (void*)0x1000;
    ConvArgs a{};
    const int prec = q[0], NT = q[1], cus = q[2], f = q[9];
    a.N = q[3]; a.H = q[4]; a.W = q[5]; a.C0 = q[6]; a.C1 = q[7]; a.Cout = q[8]; a.relu = 1;
    a.src0 = P; a.src1 = a.C1 ? P : nullptr; a.wpk = P; a.bias = (const float*)P; a.out = P;
    a.lo_delta = prec == 2 ? (int64_t)1 << 30 : 0; a.range_flag = (int*)P;
    if (f & 1) { a.res_out = P; a.res_bias = (const float*)P; }
    if (f & 2) a.plain = 1;
    if (f & 4) a.res_in = P;
    if (f & 8) a.pool_out = P;
    if (f & 16) { a.proj_w = P; a.xp0 = P; a.C0x = q[10]; a.C1x = q[11]; a.xp1 = a.C1x ? P : nullptr; }
    if (f & 32) { a.first_w = (const float*)P; a.first_b = (const float*)P; }
    if (f & 64) { a.rank1_src = (const float*)P; a.rank1_w = (const float*)P; }
    if (f & 128) { a.flat_part = (float*)P; a.flat_w4 = P; a.flat_w = P; }
    a.store_out = q[12];
    memset(out, 0, (8 + 14 + 1) * sizeof(int));
    launched[0] = 0;
    const V4Choice c = choose_v4(a, NT, cus, prec);
    out[0] = c.ok;
    strcpy(name, c.ok ? v4_form_name(c.form) : "conv3x3_v4_kernel<invalid>");
    if (!c.ok) return 0;
    const V4Form& m = c.form;
    out[1] = c.grid; out[2] = c.block; out[3] = (int)c.lds; out[4] = c.total; out[5] = c.lds_b; out[6] = a.tiles_y; out[7] = a.tiles_x;
    const int v[14] = {m.NT, m.NW, m.BRES, m.RES, m.RADD, m.POOL, m.RP, m.FIRST, m.FLAT, m.PF2, m.SPLIT, m.RANK1, m.NH, m.GRES};
    memcpy(out + 8, v, sizeof v);
    out[22] = v4_form_index(m);
    return 0;
}
int v4f_list(int* forms, int cap) {        // the list of instantiated forms, fourteen fields each
    int n = 0;
    for (const ss::V4Form& m : ss::kV4Forms) {
        if (n == cap) break;
        const int v[14] = {m.NT, m.NW, m.BRES, m.RES, m.RADD, m.POOL, m.RP, m.FIRST, m.FLAT, m.PF2, m.SPLIT, m.RANK1, m.NH, m.GRES};
        memcpy(forms + 14 * n++, v, sizeof v);
    }
    return (int)(sizeof ss::kV4Forms / sizeof ss::kV4Forms[0]);
}
}
"""


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc not found"
    d = tmp_path_factory.mktemp("v4_forms")
    src = d / "v4_forms.hip"
    src.write_text(_SRC)
    out = {}
    procs = []
    for kind, flag in (("product", []), ("dev", ["-DSS_DEVBUILD"])):
        lib = d / ("libv4_forms_%s.so" % kind)
        cmd = [hipcc, "-O1", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-fPIC", "-shared"] + flag + \
              ["-I", os.path.join(ROOT, "softspoken_amd", "csrc"), str(src), "-o", str(lib)]
        procs.append((subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), lib, kind))
    for p, lib, kind in procs:
        o, _ = p.communicate()
        assert p.returncode == 0, o
        out[kind] = str(lib)
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["product_queries"] == digest(queries()) and g["dev_queries"] == digest(dev_queries()), "the query set is not the recorded one"
    return g


def _compare(qs, got, want, where):
    assert len(got) == len(want) == len(qs)
    bad = [(q, g, w) for q, g, w in zip(qs, got, want) if g != w]
    assert not bad, "%s: %d of %d answers differ, first: query %s\n  got  %s\n  want %s" % ((where, len(bad), len(qs)) + bad[0])


def _check_forms(extra, listed):
    for name, _, rest in extra:
        if name.endswith("<invalid>"):
            continue
        form, index = rest[:14], rest[14]
        assert index >= 0 and listed[index] == form, "a supported answer's form is not in the list: " + name


def _list(lib_path):
    L = ctypes.CDLL(lib_path)
    buf = (ctypes.c_int * (14 * 512))()
    n = L.v4f_list(buf, 512)
    assert 0 < n <= 512
    return [tuple(buf[14 * i:14 * i + 14]) for i in range(n)]


def test_the_list_has_no_duplicate(libs):
    forms = _list(libs["product"])
    assert len(set(forms)) == len(forms)
    assert forms == _list(libs["dev"])                    # one instantiated set for both builds


def test_product_answers_are_the_recorded_ones(libs, golden):
    qs = queries()
    got, extra = ask(libs["product"], qs)
    _compare(qs, got, unpack(golden, "product"), "product")
    _check_forms(extra, _list(libs["product"]))
    assert sum(a is not None for a in got) > 200          # (the query set reaches the chooser's forms, it is not refused wholesale)


_CHILD = "import json, sys; sys.path.insert(0, %r); import test_v4_forms as t; a, x = t.ask(sys.argv[1], t.dev_queries()); print(json.dumps([a, x]))"


def test_dev_answers_are_the_recorded_ones_under_every_switch(libs, golden):
    """The switches are read once per process: one child per environment, all started together."""
    qs = dev_queries()
    listed = _list(libs["dev"])
    procs = []
    for e in DEV_ENVS:
        env = {k: v for k, v in os.environ.items() if not k.startswith("SOFTSPOKEN_")}
        if e:
            k, v = e.split("=")
            env[k] = v
        procs.append((e, subprocess.Popen([sys.executable, "-c", _CHILD % os.path.dirname(os.path.abspath(__file__)), libs["dev"]],
                                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)))
    for e, p in procs:
        o, err = p.communicate()
        assert p.returncode == 0, err
        got, extra = json.loads(o)
        got = [None if a is None else tuple(a) for a in got]
        _compare(qs, got, unpack(golden, "dev", e), "dev build, " + (e or "no switch"))
        _check_forms([(n, l, tuple(r)) for n, l, r in extra], listed)
