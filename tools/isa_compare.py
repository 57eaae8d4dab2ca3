"""Machine-code identity of the kernels of two builds of a HIP object:
python tools/isa_compare.py old.o new.o [...more pairs as old.o new.o]

For every kernel of new.o, the gfx950 instruction stream (llvm-objdump -d of
the extracted code object, as tools/isa_stats.py --dump; addresses, encodings
and address comments dropped) and the kernel descriptor's register, LDS,
scratch and kernarg figures (the code object's metadata notes) are compared
with the kernel of the same name in old.o.  Kernels are matched by demangled
name without the parameter list; --drop-last-arg NAME[,NAME] drops a last
template argument 0 of old.o's kernels whose name contains NAME (a removed
parameter at its default; its other values have no counterpart).
Exit status 1 if a kernel differs or has no counterpart."""
import os
import re
import subprocess
import sys
import tempfile

from isa_stats import OBJDUMP, code_objects

LLVM = os.path.dirname(OBJDUMP)
FIGURES = ("sgpr_count", "vgpr_count", "agpr_count", "sgpr_spill_count", "vgpr_spill_count",
           "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size",
           "max_flat_workgroup_size", "wavefront_size")


def kernels(path, drop):
    """{name: (instructions, figures)} of every kernel in path."""
    out = {}
    for co in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
            f.write(co)
        asm = subprocess.run([OBJDUMP, "-d", f.name], capture_output=True, text=True, check=True).stdout
        dem = subprocess.run([OBJDUMP, "-d", "--demangle", f.name], capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], capture_output=True,
                               text=True, check=True).stdout
        os.unlink(f.name)
        # amdhsa.kernels: one record per kernel, opened by "  - .", its own
        # keys (sorted, so .name comes in the middle) indented by four
        figs = {}
        for rec in re.split(r"^  - (?=\.)", notes, flags=re.M)[1:]:
            keys = dict(re.findall(r"^(?:    )?\.(\w+):\s+(\S+)$", rec, flags=re.M))
            if "name" in keys and "kernarg_segment_size" in keys:
                figs[keys["name"]] = {k: keys.get(k) for k in FIGURES}
        # the same listing demangled: the functions come in the same order
        heads = re.findall(r"^[0-9a-f]{16} <(.*)>:$", dem, flags=re.M)
        fns = re.split(r"\n(?=[0-9a-f]{16} <)", asm)
        fns = [fn for fn in fns if re.match(r"[0-9a-f]{16} <", fn)]
        assert len(heads) == len(fns), (len(heads), len(fns))
        for fn, name in zip(fns, heads):
            sym = re.match(r"[0-9a-f]{16} <(.*)>:", fn).group(1)
            if sym not in figs:
                continue
            name = name.replace("void ", "", 1)
            depth, at = 0, len(name)  # cut the parameter list: the last top-level (...)
            while at > 0:
                at -= 1
                depth += {")": 1, "(": -1}.get(name[at], 0)
                if depth == 0:
                    break
            name = name[:at] if name.endswith(")") else name
            if drop and any(d in name for d in drop.split(",")):
                name = re.sub(r", 0>$", ">", name)
            ins = [re.sub(r"\s*//.*$", "", l).strip() for l in fn.split("\n")[1:]]
            # "...": objdump's mark for the zero padding up to the next function
            out[name] = ([i for i in ins if i and i != "..."], figs[sym])
    return out


def main():
    args = sys.argv[1:]
    drop = None
    if "--drop-last-arg" in args:
        i = args.index("--drop-last-arg")
        drop = args[i + 1]
        del args[i:i + 2]
    bad = 0
    for old_path, new_path in zip(args[0::2], args[1::2]):
        old, new = kernels(old_path, drop), kernels(new_path, None)
        print(f"{os.path.basename(new_path)}: {len(old)} kernels before, {len(new)} after")
        for name, (ins, figs) in sorted(new.items()):
            if name not in old:
                verdict = "NO COUNTERPART"
            elif old[name] == (ins, figs):
                verdict = "identical"
            else:
                verdict = "DIFFERS" + (" (instructions)" if old[name][0] != ins else "") + \
                          (" (descriptor)" if old[name][1] != figs else "")
            bad += verdict != "identical"
            print(f"  {verdict:10s} {len(ins):6d} instr  vgpr {figs.get('vgpr_count')} agpr {figs.get('agpr_count')} "
                  f"sgpr {figs.get('sgpr_count')} lds {figs.get('group_segment_fixed_size')} "
                  f"scratch {figs.get('private_segment_fixed_size')} kernarg {figs.get('kernarg_segment_size')}  {name}")
        for name in sorted(set(old) - set(new)):
            print(f"  removed    {len(old[name][0]):6d} instr  {name}")
    print("RESULT:", "every remaining kernel is identical" if not bad else f"{bad} kernels differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
