"""Builds the host check programs of the K2 parse and query family (tools/k2_*_check.hip) for the tests
that run them.  A plain helper module: each test passes the headers its program compiles."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def build_check(name, tmp, headers, opt="-O1"):
    """tools/<name>, built from tools/<name>.hip and the oracle when it is missing or older than its
    sources; headers: paths from the repository's root.  tmp: a directory for the object files."""
    check = os.path.join(ROOT, "tools", name)
    src = check + ".hip"
    orc_c = os.path.join(ROOT, "oracle", "eazy_oracle.c")
    deps = [src, orc_c, os.path.join(ROOT, "oracle", "eazy_oracle.h"), os.path.join(ROOT, "include", "eazy.h")]
    deps += [os.path.join(ROOT, h) for h in headers]
    if not os.path.exists(check) or os.path.getmtime(check) < max(os.path.getmtime(d) for d in deps):
        orc_o, chk_o = str(tmp / "eazy_oracle.o"), str(tmp / (name + ".o"))
        for cmd in (["gcc", "-O2", "-std=c11", "-c", "-o", orc_o, orc_c],
                    [HIPCC, opt, "-std=c++17", "--offload-arch=gfx950", "-Wno-align-mismatch", "-c", "-o", chk_o, src],
                    [HIPCC, "-o", check, chk_o, orc_o, "-lpthread"]):
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-2000:]
    return check


def csrc(*names):
    return [os.path.join("eazy_amd", "csrc", n) for n in names]


# what every check includes: the common header and the headers behind it
COMMON = [os.path.join("tools", "k2_check_common.h")] + csrc("ez_k2_parts.h", "ez_k2_size.h", "ez_k2_parse.h", "ez_bytes.h", "ez_format.h")
