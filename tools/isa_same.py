"""Do the kernels of one source compile to the same instructions in two builds?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -Iinclude -Iadvchain_amd/csrc --cuda-device-only -S \\
          advchain_amd/csrc/loss_lp.hip -o new.s          (and the same in a checkout of the other commit: old.s)
    python tools/isa_same.py old.s new.s [--match k_lp_] [--rename OLD=NEW ...]

Kernels are paired by their demangled names (c++filt), so a template that gained a trailing, empty parameter pack pairs with
its earlier self; so does a plain kernel that became a template with nothing but such a pack (`void k<>(...)` pairs with
`k(...)`: the return type c++filt prints for templates and an empty `<>` are dropped from both names).  Compared: every instruction line with its operands, in order, and the local labels (renumbered per
function; a kernel's own constants, `__const.<mangled name>.x`, by their last part); comments and assembler directives are
dropped.  A kernel that changed its name on purpose is paired with --rename OLD=NEW (repeatable): every OLD in the demangled
names of `old.s` reads NEW before pairing, parameter list included where that changed too.  Prints one line per kernel of
`old.s` (for a kernel that differs, the new instruction count as well) and exits 1 on a kernel that differs or has no partner.
Needs no GPU."""
import argparse
import re
import subprocess
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        text = line.split(";")[0].rstrip()
        if not text.strip() or (text.strip().startswith(".") and not text.startswith(".LBB")):
            continue
        text = re.sub(r"__const\._Z\w+\.", "__const.FN.", text)     # a kernel's own constant: named after its mangled name
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", text))
    return out


def demangled(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return {n: re.sub(r"^void ", "", d).replace("<>(", "(") for n, d in zip(names, res.stdout.splitlines())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--match", default="k_lp_", help="substring of the demangled names to compare")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="replace OLD by NEW in the demangled names of `old` before pairing (repeatable)")
    args = ap.parse_args()
    old, new = functions(args.old), functions(args.new)
    old_names = demangled(list(old))
    for r in args.rename:
        a, sep, b = r.partition("=")
        if not sep or not a:
            ap.error("--rename takes OLD=NEW, got %r" % r)
        old_names = {n: d.replace(a, b) for n, d in old_names.items()}
    by_name = {d: n for n, d in demangled(list(new)).items()}
    bad = total = 0
    for o, d in sorted(old_names.items(), key=lambda kv: kv[1]):
        if args.match not in d:
            continue
        total += 1
        n = by_name.get(d)
        verdict = "no partner" if n is None else ("same" if old[o] == new[n] else "DIFFERENT")
        bad += verdict != "same"
        count = "%5d" % len(old[o]) if verdict != "DIFFERENT" else "%5d -> %d" % (len(old[o]), len(new[n]))
        print("%-10s %s instructions  %s" % (verdict, count, d[:120]))
    print("%d kernels compared, %d not the same" % (total, bad))
    sys.exit(1 if bad or not total else 0)


if __name__ == "__main__":
    main()
