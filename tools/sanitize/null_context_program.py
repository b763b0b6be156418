"""Writes a stand-alone C++ program (its own main) that makes the null-context calls of tests/decode_entry_table.py through the C
entries and compares status and message with tests/golden/decode_entry_errors.json -- for a sanitizer run of the decode host layer on
the CPU (no GPU is touched: every call is refused before the context is used):

    python tools/sanitize/null_context_program.py > /tmp/null_ctx.cpp
    cd jpezy_amd/csrc && SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
    hipcc <flags of jpezy_amd/_build.py> $SAN /tmp/null_ctx.cpp jpezy_capi*.hip jpezy_host_codec.cpp <the kernel objects> -o /tmp/null_ctx
    /tmp/null_ctx          # "N calls, 0 differ" and no sanitizer report
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "tests")]
import decode_entry_table as T  # noqa: E402


def cstr(s):
    return '"' + s.replace("\\", "\\\\").replace('"', '\\"') + '"'


def call_text(entry, over):
    a = dict(data="DATA", len="sizeof DATA", gray=0, scale=2, region=T.REGION, upsampling=T.SMOOTH, info="&info", r="OUT[0]", g="OUT[1]", b="OUT[2]",
             plane_cap="CAP", format=0, row_stride=0, pix="OUT[0]", pix_cap="CAP", y="OUT[0]", y_stride=0, y_cap="CAP", cb="OUT[1]", cr="OUT[2]",
             c_stride=0, c_step=1, c_cap="CAP", co="OUT[0]", qt="QT", ncomp=3, comp_h="ones", comp_v="ones", comp_tq="tq", precision=8,
             W=T.W, H=T.H, n_frames=1, plane_stride=T.W * T.H, frame_stride=0)
    a.update(over)
    a = {k: ("nullptr" if v is None else v) for k, v in a.items()}
    if a["co"] == "misaligned":
        a["co"] = "OUT[0] + 2"
    pre = ""
    if a["region"] != "nullptr":
        pre = "jpezy_rect rect = { %d, %d, %d, %d }; " % tuple(a["region"])
        a["region"] = "&rect"
    extra = dict(scale=a["scale"], region=a["region"], upsampling=a["upsampling"])
    co = "(const int16_t*)(%s)" % a["co"]
    if entry == "decode_jpeg_ycc":
        args = ["nullptr", a["data"], a["len"], a["info"], a["y"], a["y_stride"], a["y_cap"], a["cb"], a["cr"], a["c_stride"], a["c_step"], a["c_cap"]]
    elif entry in T.HOST_ENTRIES:
        names = T.HOST_PLANAR.get(entry, T.HOST_PACKED.get(entry))
        tail = [a["r"], a["g"], a["b"], a["plane_cap"]] if entry in T.HOST_PLANAR else [a["format"], a["row_stride"], a["pix"], a["pix_cap"]]
        args = ["nullptr", a["data"], a["len"], a["gray"]] + [extra[n] for n in names] + [a["info"]] + tail
    else:
        names = T.DEV_PLANAR.get(entry, T.DEV_PACKED.get(entry))
        head = ["nullptr", co, a["qt"], a["ncomp"], a["comp_h"], a["comp_v"], a["comp_tq"], a["precision"], a["W"], a["H"], a["gray"]]
        if names is None:
            tail = [a["r"], a["g"], a["b"], "nullptr"]
        elif entry in T.DEV_PLANAR:
            tail = [a["n_frames"], a["plane_stride"], a["r"], a["g"], a["b"], "nullptr"]
        else:
            tail = [a["format"], a["row_stride"], a["frame_stride"], a["n_frames"], a["pix"], "nullptr"]
        args = head + [extra[n] for n in names or ()] + tail
    return pre + "rc = jpezy_%s(%s);" % (entry, ", ".join(str(x) for x in args))


def main():
    want = json.loads((ROOT / "tests" / "golden" / "decode_entry_errors.json").read_text())["null_context"]
    rows = T.table("null_context")
    assert [(e, c) for e, _, c, _ in rows] == [(r["entry"], r["case"]) for r in want]
    data, _, _ = T.jpeg_synth.synth_jpeg(T.W, T.H, seed=11, **T.FILES["420"])
    out = ['#include <cstdio>', '#include <cstring>', '#include <cstdint>', '#include "%s"' % (ROOT / "include" / "jpezy_hip.h"),
           "static const uint8_t DATA[] = { %s };" % ", ".join(str(b) for b in data),
           "alignas(16) static uint8_t OUT[3][4096];", "static const size_t CAP = sizeof OUT[0];", "static uint16_t QT[4][64];",
           "static const uint8_t ones[3] = { 1, 1, 1 }, tq[3] = { 0, 1, 1 };", "static int calls = 0, differ = 0;",
           "static void check(const char* what, int rc, int status, const char* text)", "{", "    ++calls;",
           "    const char* got = rc < 0 ? jpezy_hip_last_error() : \"\";",
           "    if (rc == status && !std::strcmp(got, text)) return;", "    ++differ;",
           '    std::printf("%s: got %d \\"%s\\", recorded %d \\"%s\\"\\n", what, rc, got, status, text);', "}", "int main()", "{", "    int rc;"]
    for (entry, _, case, over), w in zip(rows, want):
        out.append("    { jpezy_frame_info info; std::memset(&info, 0, sizeof info); %s check(%s, rc, %d, %s); }"
                   % (call_text(entry, over), cstr(entry + " / " + case), w["status"], cstr(w["error"])))
    out += ['    std::printf("%d calls, %d differ\\n", calls, differ);', "    return differ != 0;", "}"]
    print("\n".join(out))


if __name__ == "__main__":
    main()
