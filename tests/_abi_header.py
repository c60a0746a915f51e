"""What the ABI tests of the side units share (tests/test_*_abi_cpu.py): the names a C header declares and the text of its
macros.  A plain helper module: it holds no test."""
import re


def declared(header_text):
    """The sbe_* functions the header declares, sorted (comments are not looked at)."""
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    return sorted(set(re.findall(r"\b(sbe_[a-z0-9_]+)\s*\(", text)))


def macro(header_text, name):
    """The replacement text of `#define name`, without its trailing comment."""
    return re.search(rf"#define {name}\s+(.+?)\s*(?:/\*|$)", header_text, flags=re.M).group(1)
