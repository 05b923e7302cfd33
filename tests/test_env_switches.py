"""The environment switches the library reads are exactly those of DESIGN.md's table (§8b): a new switch needs a row
there, a removed one loses it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "koordinator_amd", "csrc")
# a name read directly or through the helpers of gs_numa_host.h
READ = re.compile(r'\b(?:getenv|env_str|env_on|env_off|env_num)\(\s*"([^"]+)"')
ROW = re.compile(r"^\| `(GSX?_[A-Z0-9_]+)` \|", re.M)


def test_switches_read_equal_design_table():
    read = set()
    for f in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, f), encoding="utf-8") as fh:
            read.update(READ.findall(fh.read()))
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as fh:
        text = fh.read()
    table = text[text.index("### 8b. Environment switches"):text.index("## 9. ")]
    listed = set(ROW.findall(table))
    assert read and read == listed, f"read but not listed: {sorted(read - listed)}; listed but not read: {sorted(listed - read)}"
