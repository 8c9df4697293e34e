"""gs_explain's cause codes: their names, upstream's texts, and the rule that
turns the seven booleans and the pre-checks into a code, written out in plain
Python (the library's own copy is csrc/explain_rules.hpp; tests compare the
two).

<U> restated from memory of sigs.k8s.io/karpenter v1.13
(InstanceTypeFilterError.Error() and the errors of NodeClaim.CanAdd).
"""
from . import abi

CAUSE_NAMES = [
    "STATE", "NO_OPTIONS", "LIMITS", "TAINTS", "INCOMPATIBLE", "MIN_VALUES", "IT_NONE", "IT_REQ_OR_FITS",
    "IT_REQ_OR_OFFERING", "IT_FITS_OR_OFFERING", "IT_REQUIREMENTS", "IT_RESOURCES", "IT_OFFERING",
    "IT_REQ_FITS_NO_OFFERING", "IT_FITS_OFFERING_NO_REQ", "IT_REQ_OFFERING_NO_FITS", "IT_TUPLE",
]

# what upstream prints for the NodePool; None where it prints no line
CAUSE_TEXT = {
    abi.GS_WHY_STATE: None,  # a fresh NodeClaim takes the pod: the cause lay in the Solve's state
    abi.GS_WHY_NO_OPTIONS: None,  # no template, no line
    abi.GS_WHY_LIMITS: "all available instance types exceed limits for nodepool",
    abi.GS_WHY_TAINTS: "did not tolerate taint",
    abi.GS_WHY_INCOMPATIBLE: "incompatible requirements",
    abi.GS_WHY_MIN_VALUES: "minValues requirement is not met",
    abi.GS_WHY_IT_NONE: "no instance type met the scheduling requirements or had enough resources or had a "
                        "required offering",
    abi.GS_WHY_IT_REQ_OR_FITS: "no instance type met the scheduling requirements or had enough resources",
    abi.GS_WHY_IT_REQ_OR_OFFERING: "no instance type met the scheduling requirements or had a required offering",
    abi.GS_WHY_IT_FITS_OR_OFFERING: "no instance type had enough resources or had a required offering",
    abi.GS_WHY_IT_REQUIREMENTS: "no instance type met all requirements",
    abi.GS_WHY_IT_RESOURCES: "no instance type has enough resources",
    abi.GS_WHY_IT_OFFERING: "no instance type has the required offering",
    abi.GS_WHY_IT_REQ_FITS_NO_OFFERING: "no instance type which met the scheduling requirements and had enough "
                                        "resources, had a required offering",
    abi.GS_WHY_IT_FITS_OFFERING_NO_REQ: "no instance type which had enough resources and the required offering met "
                                        "the scheduling requirements",
    abi.GS_WHY_IT_REQ_OFFERING_NO_FITS: "no instance type which met the scheduling requirements and the required "
                                        "offering had the required resources",
    abi.GS_WHY_IT_TUPLE: "no instance type met the requirements/resources/offering tuple",
}

# the pre-check states of csrc/explain_rules.hpp (PRE_*)
PRE_NO_OPTIONS, PRE_LIMITS, PRE_TAINTS, PRE_INCOMPATIBLE, PRE_MIN_VALUES = (1 << i for i in range(5))


def cause_of(met, pre):
    """the table of include/gpusched.h: the first code that applies wins"""
    if pre & PRE_NO_OPTIONS:
        return abi.GS_WHY_NO_OPTIONS
    if pre & PRE_LIMITS:
        return abi.GS_WHY_LIMITS
    if pre & PRE_TAINTS:
        return abi.GS_WHY_TAINTS
    if pre & PRE_INCOMPATIBLE:
        return abi.GS_WHY_INCOMPATIBLE
    if met & abi.GS_MET_ALL:
        return abi.GS_WHY_MIN_VALUES if pre & PRE_MIN_VALUES else abi.GS_WHY_STATE
    r, f, o = met & abi.GS_MET_REQUIREMENTS, met & abi.GS_MET_FITS, met & abi.GS_MET_OFFERING
    if not r and not f and not o:
        return abi.GS_WHY_IT_NONE
    if not r and not f:
        return abi.GS_WHY_IT_REQ_OR_FITS
    if not r and not o:
        return abi.GS_WHY_IT_REQ_OR_OFFERING
    if not f and not o:
        return abi.GS_WHY_IT_FITS_OR_OFFERING
    if not r:
        return abi.GS_WHY_IT_REQUIREMENTS
    if not f:
        return abi.GS_WHY_IT_RESOURCES
    if not o:
        return abi.GS_WHY_IT_OFFERING
    if met & abi.GS_MET_REQ_FITS_ONLY:
        return abi.GS_WHY_IT_REQ_FITS_NO_OFFERING
    if met & abi.GS_MET_FITS_OFFERING_ONLY:
        return abi.GS_WHY_IT_FITS_OFFERING_NO_REQ
    if met & abi.GS_MET_REQ_OFFERING_ONLY:
        return abi.GS_WHY_IT_REQ_OFFERING_NO_FITS
    return abi.GS_WHY_IT_TUPLE


def pod_error(explained, row, nodepool_names, taints=None):
    """one pod's error as upstream words it: a list of "<NodePool>: <text>"
    lines for row `row` of an explain_to_dict result; `taints` (the problem's
    taints as (key, value, effect) texts) names the taint where one is the cause"""
    lines = []
    for t, name in enumerate(nodepool_names):
        c = int(explained["cause"][row, t])
        text = CAUSE_TEXT[c]
        if text is None:
            continue
        if c == abi.GS_WHY_TAINTS and taints is not None and explained["taint"][row, t] >= 0:
            k, v, eff = taints[int(explained["taint"][row, t])]
            text += f" {k}={v}:{eff}"
        lines.append(f"{name}: {text}")
    return lines
