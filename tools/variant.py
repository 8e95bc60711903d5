"""Build diagnostic variants of libsacenv.so from text substitutions (A/B timing only).

    python tools/variant.py name 'old text' 'new text' ['old2' 'new2' ...]
    python tools/variant.py name --src FILE     (a whole sacenv_boat.hip)
    python tools/variant.py name --file sacenv_sac_core.h 'old' 'new' ...   (that source or header only)

Copies the sources and headers to a temp dir, applies each substitution to the one file among
them (or to the file --file names) that holds its old text, which must occur exactly once -- none,
or more than one, is an error -- and builds sac-agent_amd/build/libsacenv_<name>.so.
The product sources carry no switches; variants exist only as these builds, loaded
through SACENV_LIB (never by the product path, whose library is digest-checked).
"""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def main(argv):
    name, subs = argv[0], argv[1:]
    src, target = None, None
    if subs[:1] == ["--file"]:   # the one source or header every substitution applies to
        target, subs = subs[1], subs[2:]
    if subs[:1] == ["--src"]:
        src, subs = subs[1], subs[2:]
    if len(subs) % 2:
        raise SystemExit("substitutions come in pairs")
    files = (*g.SOURCES, *g._build.HEADERS)
    with tempfile.TemporaryDirectory() as d:
        for f in files:
            shutil.copy(os.path.join(g.CSRC, f), d)
        if src:
            shutil.copy(src, os.path.join(d, target or "sacenv_boat.hip"))
        for a, b in zip(subs[::2], subs[1::2]):
            text = {f: open(os.path.join(d, f)).read() for f in ([target] if target else files)}
            hits = [f for f, s in text.items() if a in s]
            if len(hits) != 1 or text[hits[0]].count(a) != 1:
                found = ", ".join(f"{text[f].count(a)} in {f}" for f in hits) or "none"
                raise SystemExit(f"substitution must match once, in one file ({found}): {a!r}")
            open(os.path.join(d, hits[0]), "w").write(text[hits[0]].replace(a, b))
        out = os.path.join(g.BUILD, f"libsacenv_{name}.so")
        extra = os.environ.get("EXTRA_FLAGS", "").split()
        subprocess.run([g._hipcc(), *g.HIPCC_FLAGS, *extra, "-I", os.path.join(ROOT, "include"),
                        *[os.path.join(d, f) for f in g.SOURCES], "-o", out], check=True)
    print("built", out)


if __name__ == "__main__":
    main(sys.argv[1:])
