"""Shared by the CPU tests of the C ABI: what a header under include/ declares, read from its text.

    declarations("umereg_assign.h") -> {symbol: number of parameters}, in no particular order
    return_types("umereg_assign.h") -> {symbol: "int" | "size_t" | "const char*" | whatever else the header writes there}

Comments are stripped first (a comment may name an entry and an argument list).  A declaration is `umereg_<name>(` up to its closing
parenthesis; `(void)` and `()` count as no parameter, anything else as one parameter per top-level comma plus one.  Its return type is what stands in front of the name on the
declaration's line, words one space apart and every `*` attached to the word before it."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(REPO, "include")

# header -> (the module attribute that aliases its table, symbols declared): one row per header of the library
HEADERS = {
    "umereg.h": ("_lib.SIGNATURES", 77),
    "umereg_featnet.h": ("models.FEATNET_SIGNATURES", 6),
    "umereg_featnet_f16.h": ("models.FEATNET_F16_SIGNATURES", 2),
    "umereg_sparse_conv.h": ("sparse_conv.SPARSE_CONV_SIGNATURES", 6),
    "umereg_sparse_conv_f16.h": ("sparse_conv.SPARSE_CONV_F16_SIGNATURES", 1),
    "umereg_sparse_conv_pairs.h": ("sparse_conv.SPARSE_CONV_PAIRS_SIGNATURES", 2),
    "umereg_bn_act.h": ("bn_act.BN_ACT_SIGNATURES", 5),
    "umereg_ume_grad.h": ("ume_grad.UME_GRAD_SIGNATURES", 4),
    "umereg_rtume_grad.h": ("rtume_grad.RTUME_GRAD_SIGNATURES", 1),
    "umereg_gt_matches.h": ("gt_matches.GT_MATCH_SIGNATURES", 3),
    "umereg_collate.h": ("collate.COLLATE_SIGNATURES", 2),
    "umereg_assign.h": ("assign.ASSIGN_SIGNATURES", 2),
    "umereg_scan_prep.h": ("raw_scan.SCAN_PREP_SIGNATURES", 2),
    "umereg_infonce.h": ("infonce.INFONCE_SIGNATURES", 3),
    "umereg_gt_keypoints.h": ("gt_keypoints.GT_KEYPOINTS_SIGNATURES", 4),
    "umereg_icp_plane.h": ("icp_plane.ICP_PLANE_SIGNATURES", 6),
    "umereg_icp_gicp.h": ("icp_gicp.ICP_GICP_SIGNATURES", 4),
}


def text(header):
    """the header without its comments"""
    raw = open(os.path.join(INCLUDE, header)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))


def params(header, name):
    """the parameter list of `name`'s declaration as text, without the parentheses"""
    src = text(header)
    m = re.search(r"\b" + re.escape(name) + r"\s*\(", src)
    assert m, f"{name} is not declared in include/{header}"
    depth, end = 1, m.end()
    while depth:
        depth += {"(": 1, ")": -1}.get(src[end], 0)
        end += 1
    return " ".join(src[m.end():end - 1].split())


def _count(plist):
    if plist in ("", "void"):
        return 0
    depth = n = 0
    for ch in plist:
        depth += {"(": 1, ")": -1}.get(ch, 0)
        n += ch == "," and depth == 0
    return n + 1


def _names(header):
    return sorted(set(re.findall(r"\b(umereg_[a-z0-9_]+)\s*\(", text(header))))


def declarations(header):
    return {name: _count(params(header, name)) for name in _names(header)}


def return_types(header):
    src, out = text(header), {}
    for name in _names(header):
        m = re.search(r"^([^\n;(){}#]*?)\b" + re.escape(name) + r"\s*\(", src, flags=re.M)
        assert m and m.group(1).strip(), f"{name}: no return type in front of its declaration in include/{header}"
        out[name] = re.sub(r"\s*\*", "*", " ".join(m.group(1).split()))
    return out
