"""Is the gfx950 device code of two source trees the same?  For a refactor that means to touch host code only.

    python tools/device_code_identity.py PARENT_TREE CHANGE_TREE [UNIT ...] > profiles/<name>_device_code_identity.txt

Every HIP unit of alproj_amd/_build.py is compiled in both trees with the recipe's flags plus --cuda-device-only -S, the
assembly is cut into one text per function symbol (from its label to its .Lfunc_end), and the texts are compared by hash.
Local labels carry the function's ordinal in its unit (.LBB12_3), which moves when a unit's functions change order without
any instruction changing, so the ordinal and the assembler's comments (which repeat it) are dropped before hashing.  The
resource table comes from the -Rpass-analysis=kernel-resource-usage remarks of the same compilation (what
alproj_amd/_build.py: resource_usage() reads after a build).  Every unit gets one line (its function count and one digest over
all its functions' hashes and resources); the units named on the command line, and any unit that differs, are listed function by
function.  Exit code 1 when anything differs."""
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

FIELDS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def recipe(tree):
    sys.path.insert(0, tree)
    for m in [m for m in sys.modules if m.startswith("alproj_amd")]:
        del sys.modules[m]
    from alproj_amd import _build
    sys.path.pop(0)
    return _build


def compile_unit(b, src, out):
    cmd = [b.hipcc(), f"--offload-arch={b.ARCH}", "-O3", "-std=c++17", f"-I{b.INCLUDE}", f"-I{b.CSRC}"] + b.EXTRA_FLAGS.get(src, []) + \
          ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S", os.path.join(b.CSRC, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(r.stderr[-3000:])
    return " ".join(cmd), r.stderr


def functions(asm):
    """{symbol: text of its instructions and labels}"""
    out, name, body = {}, None, []
    for line in open(asm):
        m = re.match(r"^([A-Za-z_][\w.$]*):\s+; @", line)
        if m:
            name, body = m.group(1), []
        elif name and line.startswith(".Lfunc_end"):
            text = re.sub(r"[ \t]*;.*", "", "".join(body))                  # comments name loops by ordinal too
            out[name] = re.sub(r"\n+", "\n", re.sub(r"\.LBB\d+_", ".LBB_", text))
            name = None
        elif name:
            body.append(line)
    return out


def resources(remarks):
    out, cur = {}, None
    for line in remarks.splitlines():
        if "remark:" not in line:
            continue
        body = line.split("remark:", 1)[1].split("[-Rpass")[0].strip()
        if body.startswith("Function Name:"):
            cur = out.setdefault(body.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in body:
            k, v = body.split(":", 1)
            if k.strip() in FIELDS:
                cur[k.strip()] = v.strip()
    return out


def survey(tree, tmp, tag):
    b = recipe(tree)
    units = [s for s in b.SOURCES if s.endswith(".hip")]
    with ThreadPoolExecutor(4) as ex:
        res = list(ex.map(lambda s: compile_unit(b, s, os.path.join(tmp, f"{tag}_{s}.s")), units))
    return {s: (cmd, functions(os.path.join(tmp, f"{tag}_{s}.s")), resources(rem)) for s, (cmd, rem) in zip(units, res)}


def main():
    parent, change, listed = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2]), sys.argv[3:]
    tmp = os.environ.get("TMPDIR", "/tmp")
    a, b = survey(parent, tmp, "parent"), survey(change, tmp, "change")
    differ = 0
    digest = lambda t: hashlib.sha256(t.encode()).hexdigest()[:16]
    whole = lambda f, r: digest(repr(sorted((sym, digest(f[sym]), sorted(r.get(sym, {}).items())) for sym in f)))
    show = lambda cmd, tree, tag: "hipcc " + cmd.split(" ", 1)[1].replace(tree, tag).replace(tmp, "TMP")
    print("# gfx950 device code, parent against change.  Per unit: verdict, functions, digest of the whole unit (every function's\n"
          "# hash and resource usage) in parent and change.  Per function: verdict, sha256 (first 16 hex digits) of its assembly text\n"
          "# in parent and change, the change's resource usage (equal to the parent's unless noted), symbol")
    for unit in sorted(a):
        (cmd_a, fa, ra), (cmd_b, fb, rb) = a[unit], b[unit]
        unit_same = whole(fa, ra) == whole(fb, rb)
        print(f"\n{'same  ' if unit_same else 'DIFFER'} {unit}: {len(fa)} / {len(fb)} functions, {whole(fa, ra)} {whole(fb, rb)}"
              f"{'' if list(fa) == list(fb) else '; the symbols come in another order (compared per symbol)'}")
        if unit_same and unit not in listed:
            continue
        print(f"# parent: {show(cmd_a, parent, 'PARENT')}\n# change: {show(cmd_b, change, 'CHANGE')}")
        for sym in sorted(set(fa) | set(fb)):
            ha, hb = (digest(f[sym]) if sym in f else "absent" for f in (fa, fb))
            res_a, res_b = ra.get(sym, {}), rb.get(sym, {})
            same = ha == hb and res_a == res_b
            differ += not same
            table = " ".join(f"{k.split(' ')[0]}={res_b.get(k, '-')}" for k in FIELDS) if res_b else "(device function)"
            print(f"{'same  ' if same else 'DIFFER'} {ha} {hb} {table} {sym}" + ("" if res_a == res_b else f"   parent: {res_a}"))
    print(f"\n# {differ} function(s) differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
