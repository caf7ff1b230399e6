"""The ABI's extensions (include/ext/*.h) against mercury_amd/abi.py EXTENSIONS, in both directions, and against the library's exports.
tests/test_abi.py does this for the closed set under include/*.h; what the ABI gains later is declared under include/ext/ and checked here."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_HEADERS = sorted("ext/" + os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "ext", "*.h")))

SCALARS = {"int": "i", "size_t": "z", "uint64_t": "u", "long long": "q", "double": "d"}
RETURNS = {"int": "i", "void": "v", "size_t": "z", "long": "l"}
PROTOTYPE = re.compile(r"([A-Za-z_][A-Za-z_0-9 *]*?)\b(mgpu_[a-z_0-9]+)\s*\(([^()]*)\)\s*;")


def _text(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)


def _parameter(decl):
    decl = " ".join(decl.split())
    if "*" in decl or "[" in decl:
        return "s" if re.fullmatch(r"const char ?\* ?\w*", decl) else "p"
    words = [w for w in decl.split() if w != "const"]
    return SCALARS[" ".join(words[:-1]) if len(words) > 1 else words[0]]


def _return(decl):
    decl = " ".join(decl.split())
    if "*" in decl:
        return "s" if re.fullmatch(r"const char ?\*", decl) else "p"
    return RETURNS[decl]


def _prototypes(header):
    sigs = {}
    for ret, name, params in PROTOTYPE.findall(_text(header)):
        params = [] if params.strip() in ("", "void") else params.split(",")
        sig = _return(ret) + ":" + "".join(_parameter(p) for p in params)
        assert sigs.setdefault(name, sig) == sig, (header, name, "declared twice, differently")
    return sigs


def test_extension_table_matches_every_extension_header():
    from mercury_amd.abi import EXTENSIONS, PROTOTYPES
    assert EXT_HEADERS and sorted(EXTENSIONS) == EXT_HEADERS
    for header in EXT_HEADERS:
        sigs = _prototypes(header)
        called = set(re.findall(r"\b(mgpu_[a-z_0-9]+)\s*\(", _text(header)))
        assert called == set(sigs), header                                  # the prototype pattern misses no declared name
        assert EXTENSIONS[header] == sigs, (header, EXTENSIONS[header], sigs)
        for group in PROTOTYPES.values():                                   # no name is declared in both sets
            assert not set(group) & set(sigs), header
    assert EXTENSIONS["ext/mercury_excisor.h"]["mgpu_excise_dev"] == "i:ppiidppp"


def test_library_exports_and_types_every_extension():
    import ctypes as C
    from mercury_amd import abi, load_library
    lib = load_library()
    for header, sigs in abi.EXTENSIONS.items():
        assert abi.names(header) == list(sigs)
        for name, sig in sigs.items():
            assert hasattr(lib, name), "declared in include/%s but not exported: %s" % (header, name)
            restype, argtypes = abi.prototype(sig)
            fn = getattr(lib, name)
            assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert lib.mgpu_host_excise.argtypes[1] is C.c_double
