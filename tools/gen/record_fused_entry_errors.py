"""Records tests/golden/fused_entry_errors.json: what the encoder's entries and the three fused decode entries of the C-ABI answer to the
fixed table of calls in tests/fused_entry_table.py -- (entry, case, status, last_error text, SHA-256 of what a succeeding call wrote).
It is a characterisation of the library AS IT IS, so it is run against a build of the commit before a change of the host layer
(JPEZY_LIB=<that build's libjpezy_hip.so>), never against the code under test; tests/test_fused_entry_errors.py then holds the new
build to it.

    python tools/gen/record_fused_entry_errors.py            the null-context half (no GPU needed); the other half is kept
    python tools/gen/record_fused_entry_errors.py --gpu      both halves
    ... --out FILE                                           somewhere else than tests/golden/
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
FIXTURE = ROOT / "tests" / "golden" / "fused_entry_errors.json"


def main(argv):
    import jpezy_amd as J
    import fused_entry_table as T

    out = Path(argv[argv.index("--out") + 1]) if "--out" in argv else FIXTURE
    doc = json.loads(FIXTURE.read_text()) if FIXTURE.exists() else {}
    doc["null_context"] = T.Env(J).record("null_context")
    if "--gpu" in argv:
        ctx = J.Context(0)
        doc["real_context"] = T.Env(J, ctx._h).record("real_context")
        ctx.close()
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=0, sort_keys=True) + "\n")
    print(f"{out}: " + ", ".join(f"{len(v)} {k} calls" for k, v in sorted(doc.items())) + f" (library: {J.library_path()})")


if __name__ == "__main__":
    main(sys.argv[1:])
