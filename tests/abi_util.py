"""include/mmvae_hip.h as gcc sees it, for the *_abi_cpu tests that compare the ctypes binding with it."""
import os
import subprocess

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def header_facts(tmp_path, structs=None, values=None):
    """Compiles a C program against the header and returns what it printed, {key: text}: for every struct of `structs`
    ({C name: ctypes class}) "<C name>" = its sizeof and "<C name>.<field>" = the offsetof of each field the ctypes class names; for
    every item of `values` ({key: C integer expression -- a macro, an enumerator}) key = its value."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mmvae_hip.h"', "int main(void) {"]
    for cname, cls in (structs or {}).items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));' for fname, _ in cls._fields_]
    lines += [f'printf("{key} %ld\\n", (long)({expr}));' for key, expr in (values or {}).items()]
    lines.append("return 0; }")
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    return dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
