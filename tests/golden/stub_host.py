"""The boot the recorders of this directory share: a library of this project loaded over tests/golden/hip_host_stub.c instead of a HIP runtime.

    host = stub_host.boot(lib_path)      # before anything loads a HIP runtime; torch must not be imported

host._lib    signerf_amd/_lib.py, loaded by path as signerf_amd._lib (the package itself would import torch)
host.wc      tests/weights_cases.py
host.stub    the stub, built with its version script under the soname the library asks for and loaded first, so that it serves the request
host.lib     the library, every entry point of _lib's recorded headers it exports given its ctypes signature
host.args    {kernel: [bytes of each explicit argument]} from the metadata of the library's gfx950 code object, also handed to the stub,
             which needs them to log a launch's arguments (kernel_args=False: neither is done)
host.dev(n)  n bytes of the stub's arena"""
import ctypes as C, importlib.util, os, re, subprocess, sys, tempfile, types
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LLVM = "/opt/rocm/lib/llvm/bin"


def code_object(lib_path, tmp):
    """The library's gfx950 code object, extracted into tmp."""
    os.symlink(lib_path, os.path.join(tmp, "lib.so"))
    subprocess.run([LLVM + "/llvm-objdump", "--offloading", "lib.so"], cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    co, = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f]
    return os.path.join(tmp, co)


def kernel_arg_sizes(co):
    """{kernel: [bytes of each explicit argument]} from the notes of a code object."""
    notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    out, sizes, size = {}, [], 0
    for ln in notes.splitlines():
        if re.match(r"^  - \.", ln):                       # the next kernel
            sizes = []
        m = re.match(r"^      (?:- |  )\.size:\s+(\d+)", ln)
        if m:
            size = int(m.group(1))
        m = re.match(r"^      (?:- |  )\.value_kind:\s+(\S+)", ln)
        if m and not m.group(1).startswith("hidden"):
            sizes.append(size)
        m = re.match(r"^    \.name:\s+(\S+)", ln)
        if m:
            out[m.group(1)] = sizes
    return out


def boot(lib_path, kernel_args=True):
    lib_path = os.path.abspath(lib_path)
    spec = importlib.util.spec_from_file_location("signerf_amd._lib", os.path.join(ROOT, "signerf_amd", "_lib.py"))
    _lib = importlib.util.module_from_spec(spec); spec.loader.exec_module(_lib)
    pkg = types.ModuleType("signerf_amd"); pkg._lib = _lib
    sys.modules["signerf_amd"] = pkg; sys.modules["signerf_amd._lib"] = _lib
    assert "torch" not in sys.modules
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import weights_cases as wc
    tmp = tempfile.mkdtemp()
    args = kernel_arg_sizes(code_object(lib_path, tmp)) if kernel_args else {}
    stub_path = os.path.join(tmp, "libamdhip64.so.7")      # the soname the library asks for: loaded first, it satisfies that request
    subprocess.run(["gcc", "-shared", "-fPIC", "-O1", os.path.join(HERE, "hip_host_stub.c"), "-Wl,-soname,libamdhip64.so.7",
                    "-Wl,--version-script=" + os.path.join(HERE, "hip_host_stub.map"), "-o", stub_path], check=True)
    stub = C.CDLL(stub_path, mode=C.RTLD_GLOBAL)
    stub.stub_launch_name.restype = C.c_char_p
    stub.stub_launch_args.restype = C.c_size_t
    stub.stub_launch_args.argtypes = [C.c_int, C.c_void_p, C.c_size_t]
    stub.stub_launch_raw_args.restype = C.c_size_t
    stub.stub_launch_raw_args.argtypes = [C.c_int, C.c_void_p, C.c_size_t]
    lib = C.CDLL(lib_path)
    for name, (res, argtypes) in _lib.functions(recorded=True).items():
        fn = getattr(lib, name, None)      # (a reference commit's library may be older than a companion header)
        if fn is not None:
            fn.restype, fn.argtypes = res, argtypes
    for name, sizes in args.items():
        stub.stub_set_kernel_args(name.encode(), len(sizes), (C.c_uint32 * len(sizes))(*sizes))

    def dev(nbytes):
        p = C.c_void_p(None)
        assert stub.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        return p.value

    return types.SimpleNamespace(_lib=_lib, wc=wc, stub=stub, lib=lib, args=args, dev=dev)
