"""A kernel's gfx950 assembly as basic blocks, for the code-generation tests of the MLP pair kernels (tests/test_build_resources.py,
tests/test_mlp_pair256_build.py)."""
import re


def kernel_body(txt, name):
    """The text of kernel `name` in the assembly file's text: from its label to its s_endpgm."""
    i = txt.index(name + ":")
    return txt[i:txt.index("s_endpgm", i)]


def basic_blocks(body):
    """The instructions of a kernel body per basic block (split at the .LBB labels), without comments and directives."""
    blocks, cur = [], []
    for line in body.split("\n"):
        if re.match(r"^\.LBB\S+:", line):
            blocks.append(cur)
            cur = []
        else:
            ins = re.sub(r";.*", "", line).strip()
            if ins and not ins.startswith("."):
                cur.append(ins)
    blocks.append(cur)
    return blocks
