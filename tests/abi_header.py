"""What a C header of include/ declares, for the ABI tests of the five libraries (a helper module,
not a test file)."""

import re
from pathlib import Path


def strip_comments(header: Path) -> str:
    return re.sub(r"/\*.*?\*/", "", Path(header).read_text(), flags=re.S)


def functions_in(text: str, prefix: str) -> list:
    """Sorted names of the functions ``text`` (C without comments) declares whose name starts with ``prefix``."""
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(" + re.escape(prefix) + r"[a-z0-9_]+)\s*\(",
                                 text, flags=re.M)))


def declared_functions(header: Path, prefix: str) -> list:
    """Sorted names of the functions ``header`` declares whose name starts with ``prefix``."""
    return functions_in(strip_comments(header), prefix)
