"""CPU-side checks of the C-ABI: the shared library loads, and exports every symbol include/*.h declares."""
import ctypes
import glob
import os
import re

import dreamwaltz_g_amd._lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    names = set()
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        src = open(h).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        for m in re.finditer(r"\b(dwg_[a-z0-9_]+)\s*\(", src):
            names.add(m.group(1))
    return names


def test_library_exports_every_declared_symbol():
    L = _lib.lib()
    decl = _declared_symbols()
    assert decl, "no declarations found"
    for name in sorted(decl):
        assert hasattr(L, name), "libdwg_hip.so does not export %s" % name
    # and every declared symbol has a ctypes signature in the binding
    assert decl <= set(_lib.SIGNATURES), sorted(decl - set(_lib.SIGNATURES))


def test_workspace_sizes_host_only():
    L = _lib.lib()
    g, p, i = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    assert L.dwg_raster_workspace_sizes(1000, 512, 512, 5000, ctypes.byref(g), ctypes.byref(p), ctypes.byref(i)) == 0
    assert g.value >= 1000 * (48 + 8) + 3 * 1024 * 4
    assert p.value >= 5000 * 12
    assert i.value >= 512 * 512 * 8
    assert L.dwg_raster_workspace_sizes(-1, 512, 512, 0, None, None, None) != 0


def test_attention_key_split_heuristic_host_only():
    """dwg_attention_split_workspace_bytes (include/dwg_nn.h): which launches of the f32x attention split their keys over workgroups.  The SD-1.5
    sites at CFG batch 2 (8 heads): the 64x64 level's 4096 queries fill the chip (no workspace); the 32x32 level (1024 queries, 128 query
    blocks) and the 16x16 level (256 queries, 32 blocks) split; the 8x8 level has two key tiles and cross-attention three (77 keys): nothing
    to split; eight views batched (B = 16) fill the chip at 32x32 too.  Bytes = ranges x B x H x Nq x (padded head + 4) floats."""
    L = _lib.lib()
    F32X, BF16 = 3, 1
    f = L.dwg_attention_split_workspace_bytes
    assert f(F32X, 2, 8, 4096, 4096, 40) == 0
    assert f(F32X, 2, 8, 1024, 1024, 80) == 4 * 16 * 1024 * (96 + 4) * 4
    assert f(F32X, 2, 8, 256, 256, 160) == 4 * 16 * 256 * (160 + 4) * 4
    assert f(F32X, 2, 8, 64, 64, 160) == 0
    assert f(F32X, 2, 8, 1024, 77, 80) == 0
    assert f(F32X, 16, 8, 1024, 1024, 80) == 0
    assert f(BF16, 2, 8, 1024, 1024, 80) == 0          # only the split-precision unit has the merge launch
    assert f(F32X, 0, 8, 1024, 1024, 80) == 0 and f(F32X, 2, 8, 1024, 1024, 200) == 0


def test_vae_converters_and_gemm_workspace_validate_their_arguments_host_only():
    """Argument errors are reported before any device call (DWG_E_ARG), empty calls succeed: the VAE boundary converters and the split-K
    workspace of dwg_gemm_desc."""
    from dreamwaltz_g_amd import gemm
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)                    # 16-byte aligned, never dereferenced on the host
    odd = ctypes.c_void_p(4100)
    assert L.dwg_vae_image_pack(0, 512, 512, fake, fake, None) == 0 and L.dwg_vae_image_pack(1, 0, 512, fake, fake, None) == 0
    assert L.dwg_vae_image_pack(1, 8, 8, None, fake, None) != 0 and L.dwg_vae_image_pack(1, 8, 8, fake, odd, None) != 0
    assert L.dwg_vae_image_pack(-1, 8, 8, fake, fake, None) != 0
    assert L.dwg_vae_grad_prescale_pack(0, 64, fake, 64.0, fake, fake, None) != 0          # one workgroup scans the whole gradient: B >= 1
    assert L.dwg_vae_grad_prescale_pack(1, 64, fake, 64.0, fake, None, None) != 0 and L.dwg_vae_grad_prescale_pack(1, 64, fake, 64.0, odd, fake, None) != 0
    assert L.dwg_vae_dx_unpack(0, 8, 8, fake, fake, fake, None) == 0
    assert L.dwg_vae_dx_unpack(1, 8, 8, fake, None, fake, None) != 0 and L.dwg_vae_dx_unpack(1, 8, 8, odd, fake, fake, None) != 0
    # the workspace query counts whole fp32 slabs of M x N; a workspace that is not 16-byte aligned is an argument error
    d = gemm.GemmDesc()
    d.A, d.B, d.C = 4096, 8192, 12288
    d.M, d.N, d.K = 128, 1280, 11520
    d.a_row_stride, d.a_k_stride, d.b_row_stride, d.b_k_stride, d.ldc = 11520, 1, 11520, 1, 1280
    d.batch1 = d.batch2 = 1
    d.dtype, d.out_dtype, d.alpha, d.splitk = gemm.F32X, gemm.F32X, 1.0, 0
    need = L.dwg_gemm_workspace_bytes(ctypes.byref(d))
    assert need > 0 and need % (128 * 1280 * 4) == 0, need
    d.workspace, d.workspace_bytes = 4100, need
    assert L.dwg_gemm(ctypes.byref(d), None) != 0


def test_no_kernel_spills_beyond_the_known_ones():
    """The compiler's per-kernel resource report of the last build (csrc/_obj/*.resources.json, written by build.py): no kernel
    uses scratch memory except the one listed with its bound.  (Round 2 lost 7 ms per step to an epilogue change that
    silently demoted the GEMM accumulators to scratch; this is the tripwire.)"""
    from dreamwaltz_g_amd import build
    build.build(verbose=False)
    res = build.resources()
    assert sum(len(v) for v in res.values()) >= 100, "resource report missing: run python dreamwaltz-g_amd/build.py --force"
    allowed = {"k_meshbind_bwd": 128}
    bad = []
    for src, kernels in res.items():
        for name, r in kernels.items():
            scratch = r.get("ScratchSize", 0)
            if scratch == 0:
                continue
            lim = [v for k, v in allowed.items() if k in name]
            if not lim or scratch > lim[0]:
                bad.append((src, name, scratch))
    assert not bad, bad


def _c_struct_layout(header, struct, fields, tmp_path):
    """sizeof and offsetof of `struct` as the C compiler lays it out from include/<header> (the headers are plain C)."""
    import subprocess
    src = tmp_path / "layout.c"
    exe = tmp_path / "layout"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % header, 'int main(void) {',
             '  printf("%%zu\\n", sizeof(%s));' % struct]
    lines += ['  printf("%%zu\\n", offsetof(%s, %s));' % (struct, f) for f in fields]
    lines += ['  return 0; }']
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    return int(out[0]), [int(v) for v in out[1:]]


def _headers():
    return {os.path.basename(h): open(h).read() for h in sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))}


def test_ctypes_structures_have_the_layout_of_the_c_headers(tmp_path):
    """The structs that cross the C-ABI by pointer: the ctypes mirrors must agree with include/*.h field for field, for every struct the
    headers define."""
    from dreamwaltz_g_amd import gemm
    found = [(h, m) for h, src in _headers().items() for m in re.findall(r"typedef\s+struct\s+(\w+)", src)]
    assert {"dwg_nerf_field_desc", "dwg_nerf_field_grads", "dwg_scaler_state", "dwg_nerf_bg_desc", "dwg_gemm_desc"} <= {s for _, s in found}
    assert sorted(s for _, s in found) == sorted(_lib.STRUCTS)
    assert (_lib.RasterSettingsC, _lib.NerfFieldDescC, gemm.GemmDesc) == tuple(
        _lib.STRUCTS[n] for n in ("dwg_raster_settings", "dwg_nerf_field_desc", "dwg_gemm_desc"))
    for header, struct in found:
        mirror = _lib.STRUCTS[struct]
        names = [f[0] for f in mirror._fields_]
        size, offsets = _c_struct_layout(header, struct, names, tmp_path)        # a field the header lacks fails to compile
        assert size == ctypes.sizeof(mirror), (struct, size, ctypes.sizeof(mirror))
        assert offsets == [getattr(mirror, n).offset for n in names], struct
        # and the header has no field the mirror lacks: the last mirrored field ends where the struct (padding aside) ends
        last = mirror._fields_[-1]
        assert offsets[-1] + ctypes.sizeof(last[1]) + 8 > size, struct


def test_signatures_follow_the_headers_type_for_type():
    """Hand-written expectations for prototypes that between them use every mapping rule of the binding."""
    c, S = ctypes, _lib.SIGNATURES
    i32, i64, u64, f32, f64, vp = c.c_int32, c.c_int64, c.c_uint64, c.c_float, c.c_double, c.c_void_p
    assert S["dwg_image_loss_backward"] == (c.c_int, [i32] * 5 + [f64] * 2 + [vp, i64, i64, i64, i64] * 2 + [vp, vp, i32, vp, vp])
    assert S["dwg_scaler_update"] == (c.c_int, [c.POINTER(_lib.ScalerStateC), f64, f64, i32, vp])
    assert S["dwg_pc_select_above"] == (c.c_int, [u64, vp, f32, vp, u64, vp, vp, c.c_size_t, vp])
    assert S["dwg_prof_query"] == (c.c_int, [c.c_char_p, vp, vp])
    assert S["dwg_prof_dump"] == (i64, [vp, i64])                                   # a buffer the library writes: a data pointer
    assert S["dwg_grads_nonfinite_slots"] == (i32, [i64])
    assert S["dwg_gemm_workspace_bytes"] == (c.c_size_t, [c.POINTER(_lib.STRUCTS["dwg_gemm_desc"])])
    assert S["dwg_raster_num_pairs_ptr"] == (vp, [vp])                              # an int restype would truncate the address
    assert S["dwg_nerf_field_backward"] == (c.c_int, [c.POINTER(_lib.NerfFieldDescC), vp, u64, vp, vp, c.POINTER(_lib.NerfFieldGradsC), vp,
                                                      c.c_size_t, vp])
    assert S["dwg_grid_encode_forward"][1][4:10] == [c.c_uint32] * 4 + [f32, c.c_uint32]
    assert S["dwg_graph_end_capture"] == (c.c_int, [vp, vp])                        # dwg_stream_t, dwg_graph_t*
    assert len(S) == len(_declared_symbols())


def test_constants_are_the_integer_defines_of_the_headers():
    src = re.sub(r"/\*.*?\*/", "", "\n".join(_headers().values()), flags=re.S)
    defines = dict(re.findall(r"^#define[ \t]+(DWG_\w+)[ \t]*(.*?)[ \t]*$", src, flags=re.M))
    integers = {n: int(v.strip("()uU")) for n, v in defines.items() if re.fullmatch(r"\(?-?\d+[uU]?\)?", v)}
    guards = {n for n, v in defines.items() if not v}
    assert len(integers) >= 40 and len(guards) == len(_headers())
    assert _lib.CONSTANTS == integers and not guards & set(_lib.CONSTANTS)
    assert (_lib.CONSTANTS["DWG_E_ARG"], _lib.CONSTANTS["DWG_VIEW_BG_IMAGE"], _lib.CONSTANTS["DWG_ADAM_MAX_GROUPS"]) == (-1, 2, 16)
    from dreamwaltz_g_amd import condition, gemm, pointcloud
    assert (_lib.ADAM_MAX_GROUPS, condition.MAX_PEOPLE, pointcloud.MINMAX_PAIRS, gemm.F32X, gemm.ACT["geglu_pair"]) == (16, 16, 4096, 3, 6)


def test_a_declaration_the_binding_cannot_read_raises_with_its_text():
    import pytest
    for text, decl in (("int dwg_new_entry(int32_t n, half* x, dwg_stream_t stream);", "int dwg_new_entry(int32_t n, half* x, dwg_stream_t stream)"),
                       ("typedef struct dwg_new { int32_t n; long double v; } dwg_new;", "long double v"),
                       ("typedef struct dwg_new { int32_t n; complex_t v[2]; } dwg_new;", "complex_t v[2]"),
                       ("int dwg_new_entry(float x[3]);", "int dwg_new_entry(float x[3])")):
        with pytest.raises(ValueError, match=re.escape(decl)) as e:
            _lib.parse_headers({"dwg_types.h": _headers()["dwg_types.h"], "dwg_new.h": text})
        assert "dwg_new.h" in str(e.value)
    sigs, structs, consts = _lib.parse_headers({"dwg_new.h": "#define DWG_NEW_N 2\ntypedef struct dwg_new { float v[DWG_NEW_N]; } dwg_new;\n"
                                                             "void dwg_new_entry(const dwg_new* d, const char* name);"})
    assert sigs == {"dwg_new_entry": (None, [ctypes.POINTER(structs["dwg_new"]), ctypes.c_char_p])} and consts == {"DWG_NEW_N": 2}
    assert ctypes.sizeof(structs["dwg_new"]) == 8


def test_every_header_compiles_standalone_as_c_and_cxx(tmp_path):
    """include/*.h is the binding surface for a C, C++ or FFI caller: each header must stand on its own in both languages."""
    import subprocess
    for h in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        for lang, cc, std in (("c", "gcc", "-std=c99"), ("c++", "g++", "-std=c++11")):
            src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
            src.write_text('#include "%s"\nint main(void) { return 0; }\n' % os.path.basename(h))
            r = subprocess.run([cc, std, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                               capture_output=True, text=True)
            assert r.returncode == 0, (h, lang, r.stderr[:2000])
