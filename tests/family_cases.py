"""One small policy document that reaches every family set of the tile kernel, and the policy lists
drawn from it (tests/test_family_sets.py on the host, tests/test_family_sets_gpu.py on the device).

evaluate_tiles_kernel is compiled once per family set F of {image, label, container, group}
(kernels.hpp kFeat*), and plan.cpp share_fields derives F from the policy list of the pass. The
configs under configs/ reach five of the sixteen sets; the lists here reach all of them:

  plain policies   a namespace allow-list (no family bit); trusted-repos with registries, tags and
                   an image glob (image); safe-labels with denied, mandatory and constrained labels
                   (label); psp-capabilities that mutates, psp-apparmor, pod-privileged (container)
  groups           members of one family each, mixed with namespace members: a namespace-only
                   group is the group family alone
  fillers          more namespace policies, and the constant columns: invalid settings, an
                   unsupported module, a group whose expression folds to a constant

The namespace values occur in SynthBatch config 0 (a Zipf draw of ns-000.., 2 % kubewarden-approved,
3 % the always-accepted kubewarden), so namespace columns both accept and reject.
"""
import kwgpu as K

NS = "kubewarden"  # the always-accepted namespace
MOD = "registry://ghcr.io/kubewarden/policies/"
IMG, LBL, CTR, GRP, NFA, RNG = K.FEAT_IMG, K.FEAT_LBL, K.FEAT_CTR, K.FEAT_GRP, K.FEAT_NFA, K.FEAT_RNG
ALL = K.FEAT_ALL


# (each of these namespaces holds 2 to 17 of the first 197 rows of SynthBatch(0, seed=1): tests/test_family_sets.py checks)
NS_FILLERS = ["ns-1", "ns-2", "ns-ok", "ns-5", "ns-6", "ns-16", "ns-8", "ns-9", "ns-20", "ns-23"]


def _ns(value):
    return {"module": "file:///tmp/namespace-validate-policy.wasm", "settings": {"valid_namespace": value}}


def _repos(settings):
    return {"module": MOD + "trusted-repos-policy:v0.1.12", "settings": settings}


def _labels(settings):
    return {"module": MOD + "safe-labels:v0.1.14", "settings": settings}


_CAPS = {"allowed_capabilities": ["NET_ADMIN", "CHOWN", "KILL", "SETUID", "SETGID", "NET_RAW", "FOWNER", "MKNOD", "NET_BIND_SERVICE"],
         "required_drop_capabilities": ["SYS_ADMIN"], "default_add_capabilities": ["NET_BIND_SERVICE"]}
_PRIV = {"module": "registry://ghcr.io/kubewarden/tests/pod-privileged:v0.2.1"}


def document():
    doc = {
        "ns-0": _ns("ns-000"),
        "img-repos": _repos({"registries": {"allow": ["ghcr.io", "quay.io", "docker.io", "registry.k8s.io"]},
                             "tags": {"reject": ["latest", "0.*"]}, "images": {"reject": ["*/a?c*", "*@sha256:0*"]}}),
        "img-allow": _repos({"images": {"allow": ["ghcr.io/*", "quay.io/[!x]*", "*@sha256:*", "*:[1-4].*"]}}),
        "lbl-safe": _labels({"denied_labels": ["debug", "legacy"], "mandatory_labels": ["app"],
                             "constrained_labels": {"env": "^(dev|staging|prod)$", "version": "^v[0-9]+(\\.[0-9]+)*$"}}),
        "lbl-tier": dict(_labels({"mandatory_labels": ["team"], "constrained_labels": {"tier": "^(frontend|backend)$"}}),
                         policyMode="monitor"),
        "ctr-caps": {"module": MOD + "psp-capabilities:v0.1.7", "allowedToMutate": True, "settings": _CAPS},
        "ctr-aa": {"module": MOD + "psp-apparmor:v0.1.7", "settings": {"allowed_profiles": ["runtime/default", "localhost/p1"]}},
        "ctr-priv": dict(_PRIV),
        "g-ns": {"policies": {"a": _ns("ns-000"), "b": _ns("ns-002"), "c": _ns("kubewarden-approved")},
                 "expression": "a() || (b() && !c())", "message": "namespace group"},
        "g-img": {"policies": {"reg": _repos({"registries": {"allow": ["ghcr.io", "quay.io"]}}),
                               "tag": _repos({"tags": {"reject": ["latest"]}}), "n": _ns("ns-001")},
                  "expression": "(reg() && tag()) || n()", "message": "image group"},
        "g-lbl": {"policies": {"must": _labels({"mandatory_labels": ["app"]}), "deny": _labels({"denied_labels": ["pci", "critical"]}),
                               "n": _ns("ns-000")},
                  "expression": "must() && (deny() || n())", "message": "label group"},
        "g-ctr": {"policies": {"caps": {"module": MOD + "psp-capabilities:v0.1.7",
                                        "settings": {"allowed_capabilities": ["CHOWN", "KILL", "NET_ADMIN"],
                                                     "required_drop_capabilities": ["KILL"]}},
                               "priv": dict(_PRIV), "n": _ns("ns-001")},
                  "expression": "priv() && (caps() || n())", "message": "container group"},
        # fillers: no family bit
        **{name: _ns("ns-%03d" % int(name[3:])) for name in NS_FILLERS if name != "ns-ok"},
        "ns-3": _ns("ns-003"), "ns-4": _ns("ns-004"), "ns-ok": _ns("kubewarden-approved"),
        "c-bad": _repos({"registries": {"allow": ["a"], "reject": ["b"]}}),
        "c-unsupported": {"module": MOD + "verify-image-signatures:v0.2.8"},
        "c-folded": {"policies": {"a": dict(_PRIV)}, "expression": "1 + 1", "message": "constant group"},
    }
    return doc


CONSTANTS = ["c-bad", "c-unsupported", "c-folded"]
GROUPS = ["g-ns", "g-img", "g-lbl", "g-ctr"]
MUTATING = "ctr-caps"
FAMILY = {"ns": ["ns-0", "ns-3", "ns-4"], "img": ["img-repos", "img-allow"], "lbl": ["lbl-safe", "lbl-tier"],
          "ctr": ["ctr-caps", "ctr-aa", "ctr-priv"], "g_ns": ["g-ns"], "g_img": ["g-img"], "g_lbl": ["g-lbl"], "g_ctr": ["g-ctr"]}
# the family set -> what its policy list is made of
RECIPE = {
    0: ["ns"], 1: ["ns", "img"], 2: ["ns", "lbl"], 3: ["ns", "img", "lbl"], 4: ["ns", "ctr"], 5: ["ns", "img", "ctr"],
    6: ["ns", "lbl", "ctr"], 7: ["ns", "img", "lbl", "ctr"], 8: ["ns", "g_ns"], 9: ["ns", "g_img", "img"],
    10: ["ns", "g_lbl", "lbl"], 11: ["ns", "g_img", "lbl"], 12: ["ns", "g_ctr", "ctr"], 13: ["ns", "g_img", "ctr"],
    14: ["ns", "g_lbl", "ctr"], 15: ["ns", "g_img", "lbl", "ctr"],
}
SETS = sorted(RECIPE)


def selection(feat):
    """The policy list of family set `feat`: every policy of each family in its recipe."""
    return [p for fam in RECIPE[feat] for p in FAMILY[fam]]


def core(feat):
    """The narrowest list of family set `feat` (at most three columns): one policy per family, and
    the namespace policy only where nothing else is left."""
    fams = [f for f in RECIPE[feat] if f != "ns"] or ["ns"]
    return [FAMILY[fam][0] for fam in fams]


def padded(feat, width):
    """core(feat) padded with fillers to `width` columns. From width 4 on one of them is a constant
    column, at position feat % 4 of a 4-column group (the group moves with feat as well)."""
    cols = core(feat)
    if width < 4:
        return cols + NS_FILLERS[:width - len(cols)]
    cols = cols + NS_FILLERS[:width - 1 - len(cols)]
    at = feat % 4 + 4 * ((feat // 4) % (width // 4))
    cols.insert(at, CONSTANTS[feat % 3])
    assert len(cols) == width and len(set(cols)) == width
    return cols


def nfa_document():
    """One-family policies whose pattern exceeds the DFA state budget (tests/pattern_cases.py): the
    pass that reads one runs the every-family kernel with NFA elements over its narrow layout."""
    from pattern_cases import policies
    pats = policies()
    return {"ns-0": _ns("ns-000"), "img-blowup": pats["images-blowup"], "lbl-blowup": pats["labels-blowup"]}


# the batches of the device tests, as SynthBatch(config, rows, seed): three full 64-row tiles and one of
# five rows; and rows of many containers, whose 8-row tiles take predecessor ranges (cmax > 4 x rows)
DEFAULT_BATCH = (0, 197, 1)
SMALL_TILE_BATCH = (5, 200, 1)
SMALL_TILE_SETS = [1, 4, 5, 6, 7, 12, 13, 15]  # the sets with the image or the container family
TIMING_CASES = [(1, True), (9, True), (6, True), (2, True), (15, True), (2, False), (15, False)]  # (set, LDS tables)
WIDTHS = [3, 4, 8, 12]

NFA_CASES = [["img-blowup"], ["lbl-blowup"], ["ns-0", "img-blowup"], ["lbl-blowup", "ns-0"]]


def variant(feat, lds_tables, timing=False, prod=False):
    return K.Variant(feat, bool(lds_tables), bool(timing), bool(prod))


def want_variant(feat, lds_tables, timing=False, ranges=False):
    """What a single-chunk all-pairs launch of family set `feat` asks the dispatch for: the
    label / container set with LDS tables is the production shape where the verdict columns go out 16
    bytes at a time to a power-of-two number of groups (kernels.hpp tile_prod_shape; the caller passes
    prod for those), and takes the wave scan where the tiles hold predecessor ranges."""
    rng = RNG if ranges and lds_tables and feat == (LBL | CTR) else 0
    return variant(feat | rng, lds_tables, timing)


def prod_shape(feat, lds_tables, ncols, timing=False, rows_mode=False):
    """tile_prod_shape for a one-chunk launch of `ncols` columns under the default settings."""
    g = ncols // 4
    return (feat & ALL) == (LBL | CTR) and not (feat & NFA) and bool(lds_tables) and not timing and not rows_mode and \
        ncols % 4 == 0 and g >= 1 and g & (g - 1) == 0
