"""What the host tests of the C ABI share: a public header's declared functions and struct fields, the built library's exports, a C99
probe of a header's constants and layouts, and the runner of a child process that sweeps what the entry points refuse.  Plain Python:
no torch, no GPU."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def _source(header_path):
    return re.sub(r"/\*.*?\*/", "", open(header_path).read(), flags=re.S)


def declared(header_path):
    """The sorted names of the functions a header declares itself (comments and the headers it includes left out)."""
    src = re.sub(r'#include\s+"[^"]+"', "", _source(header_path))
    return sorted(set(re.findall(r"\b(sn_[a-z_0-9]+)\s*\(", src)))


def struct_fields(header_path, name):
    """The field names of ``typedef struct name {...} name;`` in declaration order."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _source(header_path), flags=re.S).group(1)
    return [re.search(r"(\w+)\s*$", ln.strip().rstrip(";")).group(1) for ln in body.split("\n") if ln.strip()]


def exported(built_lib):
    """The set of sn_* functions the built library defines and exports."""
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r" T (sn_[a-z_0-9]+)", out))


def c99_probe(tmp_path, header_file, fmt, exprs):
    """Compiles a C99 ``main`` that includes include/<header_file> (one name, or a tuple of them) and prints ``exprs`` (C source, comma
    separated) with the printf format ``fmt`` under -Wall -Werror, runs it and returns the printed words."""
    src, exe = tmp_path / "h.c", tmp_path / "h"
    includes = "".join('#include "%s"\n' % h for h in ([header_file] if isinstance(header_file, str) else header_file))
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n%sint main(void) { printf("%s\\n", %s); return 0; }\n' % (includes, fmt, exprs))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()


def refusal_sweep(script):
    """Runs ``script`` (which takes the repository root as its argument and prints one ``name result`` line per call) in a child process
    -- a crash there would be a segfault, not an exception -- and returns {name: result}."""
    r = subprocess.run([sys.executable, "-c", script, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    return dict(ln.split() for ln in r.stdout.splitlines() if len(ln.split()) == 2)
