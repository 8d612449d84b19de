"""tools/kernel_asm_diff.py on synthetic device-assembly texts: the three verdicts, symbol
renames and --must-match.  No compiler, no GPU."""
import importlib.util
import os

_PATH = os.path.join(os.path.dirname(__file__), "..", "tools", "kernel_asm_diff.py")
_spec = importlib.util.spec_from_file_location("kernel_asm_diff", _PATH)
kad = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kad)


def _kernel(sym, func_no, body, vgpr=12, scratch=0, kernarg=40):
    """One kernel as the compiler lays it out: body, descriptor, function end, comments."""
    lines = ["\t.text", "\t.globl\t%s" % sym, "\t.p2align\t8", "\t.type\t%s,@function" % sym,
             "%s:                                ; @%s" % (sym, sym), "; %bb.0:"]
    lines += [l.replace("@", str(func_no)) for l in body]
    lines += ["\ts_endpgm", "\t.section\t.rodata,\"a\",@progbits", "\t.p2align\t6, 0x0",
              "\t.amdhsa_kernel %s" % sym,
              "\t\t.amdhsa_private_segment_fixed_size %d" % scratch,
              "\t\t.amdhsa_kernarg_size %d" % kernarg,
              "\t\t.amdhsa_next_free_vgpr %d" % vgpr,
              "\t.end_amdhsa_kernel", "\t.text",
              ".Lfunc_end@:".replace("@", str(func_no)),
              "\t.size\t%s, .Lfunc_end%d-%s" % (sym, func_no, sym),
              "; NumVgprs: %d" % vgpr, ""]
    return "\n".join(lines)


BODY = ["\top_load s[2:3], s[0:1], 0x0",
        "\top_wait 0                            ; a comment",
        ".LBB@_1:                                ; =>This Inner Loop Header: Depth=1",
        "\top_mul v1, v0, v0",
        "\top_add v2, v1, v0",
        "\top_branch .LBB@_1"]
REORDERED = BODY[:3] + [BODY[4], BODY[3]] + BODY[5:]
CHANGED = BODY[:4] + ["\top_fma v2, v1, v0, v0", "\top_nop 0"] + BODY[5:]


def _verdicts(rows):
    return {sym: verdict for sym, verdict, _ in rows}


def test_three_verdicts():
    # the second file numbers its functions differently and comments differently: neither counts
    first = _kernel("k_same", 0, BODY) + _kernel("k_order", 1, BODY) + _kernel("k_changed", 2, BODY)
    second = (_kernel("k_changed", 5, CHANGED, vgpr=14, scratch=16) + _kernel("k_same", 6, BODY)
              + _kernel("k_order", 7, REORDERED)).replace("a comment", "another comment")
    rows, failed = kad.diff(first, second)
    assert _verdicts(rows) == {"k_same": "identical", "k_order": "same opcodes, order differs",
                               "k_changed": "different"}
    assert failed == []
    detail = {sym: d for sym, _, d in rows}
    assert "lines 7 -> 8" in detail["k_changed"] and "VGPR 12 -> 14" in detail["k_changed"]
    assert "scratch 0 -> 16" in detail["k_changed"] and "op_fma +1" in detail["k_changed"]
    assert "2 of 7 lines differ in place" in detail["k_order"]


def test_figures_alone_make_a_kernel_different():
    rows, _ = kad.diff(_kernel("k", 0, BODY), _kernel("k", 0, BODY, kernarg=48))
    (sym, verdict, detail), = rows
    assert verdict == "different" and "stream identical" in detail and "kernarg_size 40 -> 48" in detail


def test_rename_pairs_and_unpaired_are_reported():
    first = _kernel("k_old_any", 0, BODY) + _kernel("k_gone", 1, BODY)
    second = _kernel("k_new", 0, BODY) + _kernel("k_added", 1, BODY)
    rows, failed = kad.diff(first, second, renames=[(r"^k_old_any$", "k_new")], must_match=[r"^k_"])
    assert _verdicts(rows) == {"k_new": "identical", "k_gone": "only in the first file",
                               "k_added": "only in the second file"}
    assert sorted(failed) == ["k_added", "k_gone"]


def test_must_match_sets_the_exit_status(tmp_path, capsys):
    a, b = tmp_path / "a.s", tmp_path / "b.s"
    a.write_text(_kernel("k_same", 0, BODY) + _kernel("k_order", 1, BODY))
    b.write_text(_kernel("k_same", 3, BODY) + _kernel("k_order", 4, REORDERED))
    assert kad.main([str(a), str(b)]) == 0
    assert kad.main([str(a), str(b), "--must-match", "k_same"]) == 0
    assert kad.main([str(a), str(b), "--must-match", "k_(same|order)"]) == 1
    out = capsys.readouterr().out
    assert "k_same: identical" in out and "# must match, does not: k_order" in out
