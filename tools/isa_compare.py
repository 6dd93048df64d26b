"""Compares the gfx950 machine code of two builds of libtinyorb.so kernel by kernel.

    python tools/isa_compare.py OLD/libtinyorb.so NEW/libtinyorb.so [--ignore-template-arg=MANGLED]

Every clang offload bundle in the library's .hip_fatbin section (one per translation unit) is opened, its gfx950 code object
disassembled with llvm-objdump, and each function's instructions (encodings included, addresses and the s_nop padding after
its end dropped) compared.  Prints one line per function present in both (identical / DIFFERENT) and the functions only one
build has; exits 1 if any function present in both differs.  Cross-compiled builds suffice: no GPU is needed.

--ignore-template-arg=MANGLED (e.g. NS_12FrontGeoNoneE): a build that gave a kernel template one more, defaulted parameter names every
instance differently; the fragment is dropped from the function names, the substitution indices it shifts (S3_ -> S4_) are levelled and the
symbol a branch target is printed against is left out, so that the instances pair up and only their instructions are compared."""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def fatbin(lib):
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + f.name, lib, os.devnull])
        return open(f.name, "rb").read()


def code_objects(blob, arch="gfx950"):
    """The code objects for `arch` of every bundle in a .hip_fatbin section."""
    out, pos = [], blob.find(MAGIC)
    while pos >= 0:
        n = struct.unpack_from("<Q", blob, pos + 24)[0]
        p = pos + 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if triple.endswith(arch) or arch + ":" in triple or triple.endswith(arch + "-"):
                out.append(blob[pos + off:pos + off + size])
        pos = blob.find(MAGIC, pos + 1)
    return out


def functions(lib, ignore=None):
    """{function name: list of instruction lines without addresses} over every gfx950 code object of the library."""
    funcs = {}
    level = (lambda n: re.sub(r"S\d*_", "S_", n.replace(ignore, ""))) if ignore else (lambda n: n)
    for co in code_objects(fatbin(lib)):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", f.name], text=True)
        name = None
        for line in text.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                name = level(m.group(1))
                funcs.setdefault(name, [])
                continue
            if name and line.strip():
                # "\ts_load_dword s4, s[0:1], 0x10   // 000000001A00: C0020100 00000010" -> instruction + encoding
                ins, _, tail = line.partition("//")
                enc = tail.split(":", 1)[1].strip() if ":" in tail else ""
                if ignore:
                    enc = re.sub(r"\s*<.*>$", "", enc)  # "BF850609 <function+0x1848>": the encoding holds the offset
                funcs[name].append(ins.strip() + " | " + enc)
    for ins in funcs.values():  # the alignment padding after a function's end (its length depends on what follows it)
        while ins and ins[-1].startswith("s_nop 0 |"):
            ins.pop()
    return funcs


def main():
    ignore = next((a.split("=", 1)[1] for a in sys.argv[3:] if a.startswith("--ignore-template-arg=")), None)
    old, new = functions(sys.argv[1], ignore), functions(sys.argv[2], ignore)
    bad = 0
    for name in sorted(set(old) & set(new)):
        same = old[name] == new[name]
        bad += not same
        print("%-10s %s (%d instructions)" % ("identical" if same else "DIFFERENT", name, len(new[name])))
    for name in sorted(set(new) - set(old)):
        print("only new   %s (%d instructions)" % (name, len(new[name])))
    for name in sorted(set(old) - set(new)):
        print("only old   %s" % name)
    print("%d functions in both, %d different; %d only in the new build, %d only in the old" %
          (len(set(old) & set(new)), bad, len(set(new) - set(old)), len(set(old) - set(new))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
