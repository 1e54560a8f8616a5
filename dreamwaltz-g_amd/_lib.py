"""ctypes binding of the C-ABI in include/*.h (libdwg_hip.so).

The product path has no CPU fallback: if the HIP library is missing this module raises at first use.
"""
import ctypes
import glob
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DWG_LIB") or os.path.join(_HERE, "csrc", "libdwg_hip.so")      # DWG_LIB: an alternative build of the library (A/B experiments)
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")
_lib = None

_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
            "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_TYPE = r"(?:const\s+)?\w+(?:\s*\*(?:\s*const)?)*"          # `int32_t`, `const float*`, `float* const*`
_NAME = r"\w+(?:\[\w+\])?"                                  # a struct member: `hidden` or `weight[DWG_NERF_MAX_LAYERS]`


def _ctype(spelling, structs, handles):
    """The ctypes type of a C type as the headers spell it; ValueError for one the binding does not know."""
    words = re.sub(r"\bconst\b|\*", " ", spelling).split()
    stars = spelling.count("*")
    base = words[0] if len(words) == 1 else None
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 0 and base in handles:
        return ctypes.c_void_p
    if stars == 1 and base == "char" and "const" in spelling:
        return ctypes.c_char_p
    if stars == 1 and base in structs:
        return ctypes.POINTER(structs[base])
    if stars and (base in _SCALARS or base in handles or base in structs or base in ("void", "char", "uint8_t")):
        return ctypes.c_void_p          # every data pointer and out-parameter: takes None, c_void_p, byref(...) and ctypes arrays
    raise ValueError("unknown type %r" % spelling)


def _groups(pattern, text):
    m = re.fullmatch(pattern, text, flags=re.S)
    if m is None:
        raise ValueError("not a form the binding reads")
    return m.groups()


def parse_headers(sources):
    """({prototype name: (restype, argtypes)}, {struct name: ctypes.Structure class}, {DWG_NAME: int}) of the C headers in
    `sources`, a dict of header name -> text.  The grammar is what include/*.h uses: integer `#define DWG_*`, `typedef void* handle;`,
    `typedef struct dwg_x { type a, b; type c[DWG_N]; } dwg_x;` and prototypes of named scalar / pointer arguments.  Anything else
    raises ValueError with the header and the declaration: nothing is skipped or guessed."""
    constants, handles, bodies, structs, signatures, rest = {}, set(), [], {}, {}, []

    def declaration(header, text, parse):
        try:
            parse(text)
        except ValueError as e:
            raise ValueError("%s: cannot bind the declaration `%s` (%s)" % (header, " ".join(text.split()), e)) from None

    for header, text in sorted(sources.items()):
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
        for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(DWG_\w+)[ \t]+\(?(-?\d+)[uU]?\)?[ \t]*$", text, flags=re.M):
            constants[name] = int(value)
        text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)
        text, wrapped = re.subn(r'extern\s+"C"\s*\{', " ", text)
        if wrapped:
            text = text.rstrip()
            if not text.endswith("}"):
                raise ValueError('%s: the extern "C" block is not closed at the end of the header' % header)
            text = text[:-1]
        bodies += [(header,) + m for m in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S)]
        text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
        for decl in filter(None, (d.strip() for d in text.split(";"))):
            m = re.fullmatch(r"typedef\s+void\s*\*\s*(\w+)", decl)
            if m:
                handles.add(m.group(1))
            else:
                rest.append((header, decl))

    def struct(header, tag, body, name):
        def parse(decl):
            ctype, names = _groups(r"(%s)\s*(%s(?:\s*,\s*%s)*)" % (_TYPE, _NAME, _NAME), decl)
            names = [n.strip() for n in names.split(",")]
            if "*" in ctype and len(names) > 1:
                raise ValueError("one pointer member per declaration")
            ctype = _ctype(ctype, (), handles)      # a struct nested in a struct is not in the grammar
            for n in names:
                n, _, dim = n.rstrip("]").partition("[")
                fields.append((n, ctype * (constants[dim] if dim in constants else int(dim)) if dim else ctype))
        fields = []
        if tag != name:
            raise ValueError("%s: struct %s is typedef'ed as %s" % (header, tag, name))
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            declaration(header, decl, parse)
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": "struct %s (include/%s)." % (name, header)})

    def prototype(decl):
        res, name, args = _groups(r"(%s)\s*(dwg_\w+)\s*\((.*)\)" % _TYPE, decl)
        args = [] if args.strip() == "void" else [_groups(r"(%s)\s*\w+" % _TYPE, a.strip())[0] for a in args.split(",")]
        signatures[name] = (None if res == "void" else _ctype(res, structs, handles), [_ctype(a, structs, handles) for a in args])

    for b in bodies:
        struct(*b)
    for header, decl in rest:
        declaration(header, decl, prototype)
    return signatures, structs, constants


def _read_headers():
    sources = {}
    for h in glob.glob(os.path.join(INCLUDE_DIR, "*.h")):
        with open(h) as f:
            sources[os.path.basename(h)] = f.read()
    if not sources:
        raise RuntimeError("no C headers in %s: the binding is derived from include/*.h next to the package" % INCLUDE_DIR)
    return sources


# include/*.h is the only statement of the ABI: name -> (restype, argtypes) of every prototype, a ctypes mirror of every struct, and every
# integer #define DWG_*
SIGNATURES, STRUCTS, CONSTANTS = parse_headers(_read_headers())

RasterSettingsC, RasterFramesC = STRUCTS["dwg_raster_settings"], STRUCTS["dwg_raster_frames"]
AdamGroupC, SegmentC, ScalerStateC = STRUCTS["dwg_adam_group"], STRUCTS["dwg_segment"], STRUCTS["dwg_scaler_state"]
NerfFieldDescC, NerfFieldGradsC = STRUCTS["dwg_nerf_field_desc"], STRUCTS["dwg_nerf_field_grads"]
NerfBgDescC, NerfBgGradsC = STRUCTS["dwg_nerf_bg_desc"], STRUCTS["dwg_nerf_bg_grads"]
ADAM_MAX_GROUPS, SCALER_MAX_SLOTS = CONSTANTS["DWG_ADAM_MAX_GROUPS"], CONSTANTS["DWG_SCALER_MAX_SLOTS"]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libdwg_hip.so not found at %s -- run `python dreamwaltz-g_amd/build.py` "
                "(there is no CPU fallback for the product path)" % LIB_PATH)
        # torch first: its wheel bundles its own libamdhip64 / libhsa-runtime64, and libdwg_hip.so (linked against /opt/rocm's
        # libamdhip64.so.7) must bind to THAT already-loaded runtime -- loaded the other way round the process ends up with two HIP
        # runtimes and every launch on a torch stream fails with DWG_E_LAUNCH.
        import torch  # noqa: F401
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed with DWG error %d" % (what, rc))


def ptr(t):
    """Device (or host) address of a torch tensor, None -> NULL."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream(x):
    """The current HIP stream of a tensor's device (or of a device) as a dwg_stream_t argument."""
    return ctypes.c_void_p(torch.cuda.current_stream(getattr(x, "device", x)).cuda_stream)


def check_tensor(name, t, dtype=torch.float32, shape=None, numel=None, contiguous=True, device=None):
    """RuntimeError unless t is a CUDA tensor of `dtype` (one or a tuple), of `shape` (None entries: any extent) or of `numel` elements,
    contiguous unless contiguous=False, and on `device` when one is given.  The wrappers call it before any launch."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError("%s must be a tensor, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)
    if t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)):
        raise RuntimeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if shape is not None and (t.dim() != len(shape) or any(s is not None and t.shape[k] != s for k, s in enumerate(shape))):
        raise RuntimeError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    if numel is not None and t.numel() != numel:
        raise RuntimeError("%s has %d elements, expected %d" % (name, t.numel(), numel))
    if contiguous and not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)
    if device is not None and t.device != device:
        raise RuntimeError("%s is on %s, expected %s" % (name, t.device, device))


def prof_enable(on=True):
    check(lib().dwg_prof_enable(int(bool(on))), "dwg_prof_enable")


def prof_table():
    """{kernel name: (launches, total_ms)} recorded since prof_enable(True)."""
    L = lib()
    need = L.dwg_prof_dump(None, 0)
    buf = ctypes.create_string_buffer(int(need) + 16)
    L.dwg_prof_dump(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        n, c, ms = line.split()
        out[n] = (int(c), float(ms))
    return out


def prof_symbols():
    """{kernel symbol (as rocprofv3 lists it): (launches, total_ms, algorithmic work)} since prof_enable(True)."""
    L = lib()
    need = L.dwg_prof_dump_symbols(None, 0)
    buf = ctypes.create_string_buffer(int(need) + 16)
    L.dwg_prof_dump_symbols(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        n, c, ms, w = line.split("\t")
        out[n] = (int(c), float(ms), float(w))
    return out
