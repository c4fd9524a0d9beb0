"""tools/kernel_isa_hash.py on miniature assembly: what a code move may change (a kernel's file, its position, the function index in its
local labels, comments) leaves the hashes alone; an instruction or a metadata field does not; a kernel in two files is reported."""
import importlib.util
import os

_SPEC = importlib.util.spec_from_file_location(
    "kernel_isa_hash", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "kernel_isa_hash.py"))
kih = importlib.util.module_from_spec(_SPEC)
_SPEC.loader.exec_module(kih)


def _kernel(sym, f, op="v_add_f32_e32 v0, v1, v2"):
    return """\t.text
\t.protected\t%(s)s ; -- Begin function %(s)s
\t.globl\t%(s)s
\t.type\t%(s)s,@function
%(s)s:                                  ; @%(s)s
; %%bb.0:
\t.loc\t1 %(f)d 0
\ts_cbranch_scc1 .LBB%(f)d_2
; %%bb.1:
\t%(op)s ; a remark
.LBB%(f)d_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel %(s)s
\t\t.amdhsa_next_free_vgpr 3
\t.end_amdhsa_kernel
\t.text
.Lfunc_end%(f)d:
\t.size\t%(s)s, .Lfunc_end%(f)d-%(s)s
                                        ; -- End function
""" % {"s": sym, "f": f, "op": op}


def _meta(sym, vgprs=3):
    return """  - .agpr_count:     0
    .args:
      - .name:           a
        .offset:         0
        .size:           8
    .name:           %s
    .vgpr_count:     %d
""" % (sym, vgprs)


def _file(kernels, metas, ident="clang 1"):
    return ("\t.file\t\"x.hip\"\n" + "".join(kernels) + "\t.ident\t\"%s\"\n\t.amdgpu_metadata\n---\namdhsa.kernels:\n" % ident
            + "".join(metas) + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\t.end_amdgpu_metadata\n")


def test_kernel_hashes_follow_the_code_not_its_place(tmp_path):
    both = kih.kernel_hashes(_file([_kernel("k_a", 0), _kernel("k_b", 1)], [_meta("k_a"), _meta("k_b")]))
    alone = kih.kernel_hashes(_file([_kernel("k_b", 0)], [_meta("k_b")], ident="clang 2"))
    assert set(both) == {"k_a", "k_b"} and set(alone) == {"k_b"}
    assert both["k_b"] == alone["k_b"]                    # second in one file, first in the other: other label indices, same hashes
    assert both["k_a"][0] != both["k_b"][0]               # (the symbol is part of the text)

    other_op = kih.kernel_hashes(_file([_kernel("k_b", 0, op="v_sub_f32_e32 v0, v1, v2")], [_meta("k_b")]))
    assert other_op["k_b"][0] != alone["k_b"][0] and other_op["k_b"][1] == alone["k_b"][1]
    other_meta = kih.kernel_hashes(_file([_kernel("k_b", 0)], [_meta("k_b", vgprs=4)]))
    assert other_meta["k_b"][0] == alone["k_b"][0] and other_meta["k_b"][1] != alone["k_b"][1]

    assert kih.clean('\t.asciz\t"a;b" ; remark') == ['\t.asciz\t"a;b"']   # a ';' inside a string is text, not a comment
    assert kih.clean('\t.asciz\t"a\\";b" ; remark') == ['\t.asciz\t"a\\";b"']

    paths = {}
    for name, text in (("before", _file([_kernel("k_a", 0), _kernel("k_b", 1)], [_meta("k_a"), _meta("k_b")])),
                       ("one", _file([_kernel("k_b", 0), _kernel("k_a", 1)], [_meta("k_b"), _meta("k_a")])),
                       ("two", _file([_kernel("k_b", 0)], [_meta("k_b")])),
                       ("a_only", _file([_kernel("k_a", 0)], [_meta("k_a")])),
                       ("b_changed", _file([_kernel("k_b", 0, op="v_sub_f32_e32 v0, v1, v2")], [_meta("k_b")]))):
        paths[name] = str(tmp_path / (name + ".s"))
        with open(paths[name], "w") as fh:
            fh.write(text)
    load = lambda *names: kih.load([paths[n] for n in names])[0]
    assert kih.compare(load("before"), load("a_only", "two")) == ([], [], [], [])
    assert kih.main(["--before", paths["before"], "--after", paths["a_only"], paths["two"]]) == 0
    assert kih.compare(load("before"), load("one", "two")) == ([], [], ["k_b"], [])      # k_b sits in both "after" files
    assert kih.main(["--before", paths["before"], "--after", paths["one"], paths["two"]]) == 1
    assert kih.compare(load("before"), load("a_only")) == (["k_b"], [], [], [])
    assert kih.compare(load("a_only"), load("before")) == ([], ["k_b"], [], [])
    assert kih.compare(load("before"), load("a_only", "b_changed")) == ([], [], [], ["k_b"])
    assert kih.main(["--before", paths["before"], "--after", paths["a_only"], paths["b_changed"]]) == 1
