"""What the C-ABI tests share (no GPU): a parser for the headers under include/, the map from C types to ctypes, the one
gcc command line that compiles a C host program against the library, and the library's exported symbols.
tests/test_abi_headers.py applies them to every header of _lib.HEADERS; the tests/test_*_abi.py files keep what is
specific to their header."""
import ctypes
import functools
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


@functools.lru_cache(maxsize=None)
def built_lib():
    """plnerf_amd._lib, with the library built first if it is absent."""
    if not os.path.exists(os.path.join(ROOT, "pl-nerf_amd", "libplnerf_hip.so")):
        import __graft_entry__ as ge
        ge.build()
    from plnerf_amd import _lib
    return _lib


def _code(header_path):
    return re.sub(r"/\*.*?\*/", "", open(header_path).read(), flags=re.S)


def prototypes(header_path):
    """{name: (return type, [parameter types])} of every entry point the header declares (comments stripped)."""
    protos = {}
    for ret, name, args in re.findall(r"^(int|size_t|const char\*)\s+(plnerf_\w+)\s*\(([^;]*?)\)\s*;", _code(header_path),
                                      flags=re.M | re.S):
        params = [a.strip() for a in " ".join(args.split()).split(",")]
        protos[name] = (ret, [re.match(r"^(.*?)\b\w+$", a).group(1).strip() for a in params if a != "void"])
    return protos


def structs(header_path):
    """{typedef name: [(field type, field name, array length or None)]}, fields in declaration order."""
    out = {}
    for body, name in re.findall(r"typedef struct \w+ \{(.*?)\}\s*(\w+);", _code(header_path), flags=re.S):
        fields = (re.match(r"^(.*?)\b(\w+)(?:\[(\w+)\])?$", " ".join(d.split())) for d in body.split(";") if d.strip())
        out[name] = [(m.group(1).strip(), m.group(2), m.group(3)) for m in fields]
    return out


SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
           "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}
# (on LP64 size_t and uint64_t are one ctypes object, and so are unsigned and uint32_t)
_CLASSES = {ctypes.c_int: "i32", ctypes.c_uint32: "u32", ctypes.c_float: "f32", ctypes.c_double: "f64",
            ctypes.c_uint64: "u64", ctypes.c_int64: "i64"}


def bare(c_type):
    return c_type.replace("const ", "").replace("const*", "*").strip()


def c_class(c_type):
    """ABI class of a C parameter or return type: ptr, i32, u32, i64, u64, f32 or f64."""
    t = bare(c_type)
    return "ptr" if t.endswith("*") or t == "plnerf_stream_t" else _CLASSES[SCALARS[t]]


def ct_class(ct):
    """ABI class of a ctypes type."""
    if ct is ctypes.c_char_p or ct is ctypes.c_void_p or (isinstance(ct, type) and issubclass(ct, ctypes._Pointer)):
        return "ptr"
    return _CLASSES[ct]


@functools.lru_cache(maxsize=None)
def abi_structs():
    """{typedef name: ctypes.Structure} over every header of _lib.HEADERS."""
    return {name: mirror for _, _, mirrors in built_lib().HEADERS for name, mirror in mirrors.items()}


def expected_ctype(c_type, length=None):
    """The ctypes type that mirrors a struct field of C type `c_type` (an array of `length` elements unless None): a scalar,
    one of the ABI's structs by value, or c_void_p for any pointer."""
    t = bare(c_type)
    if t in abi_structs():
        base = abi_structs()[t]
    elif c_class(t) == "ptr":
        base = ctypes.c_void_p
    else:
        base = SCALARS[t]
    if length is None:
        return base
    return base * ({"PLNERF_N_PARAM_TENSORS": built_lib().N_PARAM_TENSORS}.get(length) or int(length))


def compile_c(source, out_dir, name):
    """Compile a C99 host program (the path of an existing .c file, or else the program's text) against include/ and the
    built library; returns the executable's path."""
    if not os.path.isfile(str(source)):
        path = os.path.join(str(out_dir), name + ".c")
        with open(path, "w") as f:
            f.write(source)
        source = path
    exe = os.path.join(str(out_dir), name)
    libdir = os.path.dirname(built_lib().LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INCLUDE, str(source), "-o", exe, "-L", libdir,
                    "-lplnerf_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=120)
    return exe


def exported_symbols(lib_path):
    """The dynamic symbols the shared library defines."""
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True, timeout=120).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}
