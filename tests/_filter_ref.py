"""misopy/filter_events.py's row test (:241-327) and replicate vote (:122-176) restated for Python 3, as the reference
writes them: explicit ifs, the same helper split, its own counts regex.  Independent of miso_amd/filter_events.py
(nothing is imported from the product).  Test infrastructure only.

A table is read into dicts of strings; the selection is a list of row indices per table, so that a test can compare it with
the lines of a `.filtered` file."""
import re
from collections import defaultdict


def read_table(path):
    with open(path) as f:
        lines = [ln for ln in f.read().split("\n") if ln.strip()]
    if not lines:
        return [], []
    head = lines[0].split("\t")
    return head, [dict(zip(head, ln.split("\t"))) for ln in lines[1:]]


def get_counts(counts_str):                                  # :27-58
    num_inc = num_exc = num_both = 0
    fields = re.findall(r"(\(.{3}\):\d+)", counts_str)
    for field in fields:
        iso_type, count = field.split(":")
        count = int(count)
        if iso_type == "(1,0)":
            num_inc = count
        elif iso_type == "(0,1)":
            num_exc = count
        elif iso_type == "(1,1)":
            num_both = count
    return num_inc, num_exc, num_both


def filter_event(sample_inc, sample_exc, sample_both, num_total, num_inc, num_exc, num_sum):   # :61-81
    for have, want in ((sample_inc + sample_exc + sample_both, num_total), (sample_inc + sample_exc, num_sum),
                       (sample_inc, num_inc), (sample_exc, num_exc)):
        if have < want:                                      # the reference rejects on `<`: equality passes
            return False
    return True


def filter_events(rows, num_total=0, num_inc=0, num_exc=0, num_sum=0, delta_psi_filter=0, bf_filter=0,
                  apply_both_samples=False):                 # :241-327
    if abs(delta_psi_filter) > 1:
        raise Exception("Error: delta psi value outside [0, 1].")
    passed = []
    for idx, event in enumerate(rows):
        delta_psi = float(event["diff"])
        bayes_factor = min(float(event["bayes_factor"]), 1e12)
        s1 = filter_event(*get_counts(event["sample1_counts"]), num_total, num_inc, num_exc, num_sum)
        s2 = filter_event(*get_counts(event["sample2_counts"]), num_total, num_inc, num_exc, num_sum)
        if abs(delta_psi) < abs(delta_psi_filter):
            continue
        if abs(bayes_factor) < abs(bf_filter):
            continue
        if apply_both_samples:
            if not s1 or not s2:
                continue
        else:
            if not s1 and not s2:
                continue
        passed.append(idx)
    return passed


def multi_filter(tables, vote_thresh=0, same_direction=False, **thresholds):
    """tables: lists of row dicts.  -> per table the indices of the rows the reference writes (:109-185)."""
    comp = [filter_events(rows, **thresholds) for rows in tables]
    if len(comp) == 1:
        return comp
    event_dict = defaultdict(list)
    for rows, passed in zip(tables, comp):
        for idx in passed:
            event_dict[rows[idx]["event_name"]].append(rows[idx])
    for name in list(event_dict):
        if len(event_dict[name]) < vote_thresh:
            del event_dict[name]
            continue
        if same_direction:                                   # the opt-in the reference's comment at :138 describes
            up = sum(1 for ev in event_dict[name] if float(ev["diff"]) > 0)
            down = sum(1 for ev in event_dict[name] if float(ev["diff"]) < 0)
            if up < vote_thresh and down < vote_thresh:
                del event_dict[name]
    return [[idx for idx in passed if rows[idx]["event_name"] in event_dict] for rows, passed in zip(tables, comp)]
