"""The store policy: what needs no device -- the ABI surface, the setter's refusal of unknown bits, the default a new
context takes (the one profiles/store_policy/README.md says was adopted) and the parsing of LGCN_STORE_POLICY."""
import os
import re

import pytest

from conftest import REPO

NEW_SYMBOLS = ("lgcn_ctx_set_store_policy", "lgcn_ctx_get_store_policy")


def test_new_symbols_in_header_binding_and_library(pkg):
    hdr = open(os.path.join(REPO, "include", "lgcn_hip.h")).read()
    assert int(re.search(r"#define\s+LGCN_ABI_VERSION\s+(\d+)", hdr).group(1)) == 13      # additive: the ABI stays 13
    declared = set(re.findall(r"\b(lgcn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    lib = pkg._lib.load()
    assert lib.lgcn_abi_version() == 13
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(lib, name), name
    for name, value in (("LGCN_STORE_ADAM", pkg._lib.STORE_ADAM), ("LGCN_STORE_XLAST", pkg._lib.STORE_XLAST),
                        ("LGCN_STORE_ARG_MV", pkg._lib.STORE_ARG_MV), ("LGCN_STORE_ARG_P", pkg._lib.STORE_ARG_P),
                        ("LGCN_STORE_ARG_Y", pkg._lib.STORE_ARG_Y)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1)) == value, name


def test_setter_refuses_unknown_bits(pkg):
    lib = pkg._lib.load()
    for bits in (4, 7, 8, -1, 1 << 20):                 # refused for what they are, before the context is looked at
        assert lib.lgcn_ctx_set_store_policy(None, bits) == 3
        assert b"unknown store policy bits" in lib.lgcn_last_error()
    for bits in (0, 1, 2, 3):
        assert lib.lgcn_ctx_set_store_policy(None, bits) == 3
        assert b"null context" in lib.lgcn_last_error()


def _adopted():
    """the policy profiles/store_policy/README.md says the library ships with"""
    text = open(os.path.join(REPO, "profiles", "store_policy", "README.md")).read()
    m = re.search(r"^\*\*Adopted default: policy (\d)\b", text, flags=re.M)
    assert m, "the README states the adopted default on a line of its own"
    return int(m.group(1))


def test_default_is_the_adopted_one(pkg, monkeypatch):
    monkeypatch.delenv("LGCN_STORE_POLICY", raising=False)
    assert pkg._lib.load().lgcn_ctx_get_store_policy(None, None) == _adopted()


@pytest.mark.parametrize("text,want", [("0", 0), ("1", 1), ("2", 2), ("3", 3), ("4", -1), ("", -1), ("on", -1), ("-1", -1),
                                       ("11", -1), (" 1", -1), ("1 ", -1), ("0x1", -1)])
def test_environment_variable_parses(pkg, monkeypatch, text, want):
    """0..3 are taken; anything else is an error of lgcn_ctx_create (rc 3), reported here as -1"""
    monkeypatch.setenv("LGCN_STORE_POLICY", text)
    assert pkg._lib.load().lgcn_ctx_get_store_policy(None, None) == want
