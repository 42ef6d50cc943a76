"""CPU checks of the device-memory contract ("device memory: payload, slack, red zones"): the runtime's
allocator is called from one place, so that the registry and the red zones of GPE_FLAG_GUARD_ALLOCS see every buffer."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-physics-engine_amd", "csrc")


def _code(path):
    """The file without its comments (string literals here hold no comment markers that matter to the scan)."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")))


def test_device_allocation_has_one_home():
    """hipMalloc( and hipFree( occur in gpe_api.hip only (gpe_dev_reserve / gpe_dev_release and the checker's own
    scratch); every other file goes through them.  No other device allocator is used anywhere."""
    hits = {}
    for path in _sources():
        code = _code(path)
        for call in ("hipMalloc", "hipFree", "hipMallocAsync", "hipFreeAsync", "hipMallocManaged", "hipExtMallocWithFlags",
                     "hipMallocPitch", "hipMalloc3D", "hipMallocFromPoolAsync"):
            if re.search(r"\b%s\(" % call, code):
                hits.setdefault(call, []).append(os.path.basename(path))
    assert hits == {"hipMalloc": ["gpe_api.hip"], "hipFree": ["gpe_api.hip"]}, hits


def test_pinned_host_memory_stays_where_it_was():
    """hipHostMalloc: the two pinned mirrors (the native step's statistics, the sharded exchange's counts), nothing else."""
    hits = sorted(os.path.basename(p) for p in _sources() if re.search(r"\bhipHostMalloc\(", _code(p)))
    assert hits == ["gpe_native.hip", "k_shard.hip"], hits


TAG = (r'"(?:particles|grid|uid|remove|query|user|sort|scan|onesweep|native|shard|ctl|group'
       r'|contacts|clusters|ray|nearest|spawn|edit|tracers|monitor)\.[a-z0-9_]+"')


def _calls(code, name):
    """The argument text of every call of `name(` in code (balanced parentheses), definitions and declarations aside."""
    out = []
    for m in re.finditer(r"(?<![\w:])%s\(" % name, code):
        line_start = code.rfind("\n", 0, m.start()) + 1
        head = code[line_start:m.start()]
        if re.search(r"\b(static|inline|hipError_t|gpe_status|void)\s+$", head):  # a definition / declaration
            continue
        depth, i = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(code[i], 0)
            i += 1
        out.append(" ".join(code[m.end():i - 1].split()))
    return out


def test_every_allocation_site_names_a_tag():
    """Every call of an allocating helper (gpe_dev_reserve, dev_reserve, dev_alloc, ws_alloc, a set upload's
    up.reserve, node_table_upload, gpe_edits.hip's edit_buffer, gpe_native.hip's reserve, ensure_words) ends in a tag: a literal of the registry's naming scheme, or an expression made of such literals
    (a choice between tags), or the tag parameter a wrapper hands on.  No tag is longer than gpe_guard_zone.tag holds."""
    sites, tags = 0, set()
    for path in _sources():
        code = _code(path)
        names = ["gpe_dev_reserve", "dev_reserve", "dev_alloc", "ws_alloc", r"up\.reserve", "edit_buffer", "ensure_words",
                 "cell_grid_upload", "sweep_mode_set", "node_table_upload"]   # (the last three hand their tags on to up.reserve)
        if os.path.basename(path) == "gpe_native.hip":
            names.append("reserve")
        for name in names:
            for args in _calls(code, name):
                last = args.rsplit(",", 1)[1].strip() if "," in args else args
                # (a ?: choice between tags holds no comma; its literals are what counts)
                found = re.findall(TAG, args.split(",", 3)[-1] if name != "ensure_words" else last)
                assert found or last in ("tag", "t.tag", "cell_start_tag", "items_tag", "b.second", "node_uid_tag",
                                         "node_slot_tag", "row_start_tag"), (os.path.basename(path), name, args)
                sites += 1
                tags.update(t.strip('"') for t in found)
    assert sites >= 127, sites
    assert all(len(t) < 32 for t in tags), sorted(tags)          # gpe_guard_zone.tag is char[32]


def _body(code, name):
    """The body of the function `name` defined at the left margin of code."""
    m = re.search(r"^[\w:<> \*]*\b%s\([^{;]*\)\n\{\n(.*?)\n\}" % re.escape(name), code, flags=re.S | re.M)
    assert m, name
    return m.group(1)


# workspace: (file, the functions that allocate its buffers, its release function)
WORKSPACES = {
    "remove": ("gpe_api.hip", ["remove_reserve"], "remove_release"),
    "uid": ("gpe_api.hip", ["alloc_particle_buffers", "uids_switch_on", "uid_map_build", "uid_query_reserve"], "uid_release"),
    "query": ("gpe_queries.hip", ["query_reserve"], "gpe::query_release"),
    "contacts": ("gpe_queries.hip", ["contacts_reserve"], "gpe::contacts_release"),
    "clusters": ("gpe_queries.hip", ["clusters_reserve"], "gpe::clusters_release"),
    "ray": ("gpe_queries.hip", ["ray_reserve"], "gpe::ray_release"),
    "nearest": ("gpe_queries.hip", ["nearest_reserve"], "gpe::nearest_release"),
    "spawn": ("gpe_edits.hip", ["spawn_reserve"], "gpe::spawn_release"),
    "edit": ("gpe_edits.hip", ["do_edit", "do_kick"], "gpe::edit_release"),
    "tracers": ("gpe_observe.hip", ["gpe_tracers_begin"], "tracers_release"),
    "monitor": ("gpe_observe.hip", ["monitor_reserve", "gpe_monitor_begin"], "monitor_release"),
}


def test_every_workspace_releases_exactly_what_it_reserves():
    """For each workspace the fields its reserve functions allocate (the pointer handed to dev_alloc / ws_alloc /
    edit_buffer / a set upload's up.reserve, next to a tag of that workspace) are the fields its release function hands to dev_free, no more and no
    fewer -- and free_particle_buffers / observers_release call every release function."""
    api = _code(os.path.join(CSRC, "gpe_api.hip"))
    observe = _code(os.path.join(CSRC, "gpe_observe.hip"))
    callers = _body(api, "free_particle_buffers") + _body(observe, "gpe::observers_release")
    for prefix, (fname, reserves, release) in WORKSPACES.items():
        code = _code(os.path.join(CSRC, fname))
        reserved = set()
        for fn in reserves:
            for name in ("dev_alloc", "ws_alloc", "edit_buffer", r"up\.reserve"):
                for args in _calls(_body(code, fn), name):
                    tag = re.search(r'"%s\.([a-z0-9_]+)"' % prefix, args)
                    if not tag:
                        continue                                        # (another owner's buffer)
                    field = re.search(r"&[\w>.-]*?(\w+),", args).group(1)
                    assert field == tag.group(1), (prefix, args)          # the tag names the field
                    reserved.add(field)
        freed = re.findall(r"dev_free\(c, [\w>.-]*?(\w+)\)", _body(code, release))
        assert len(freed) == len(set(freed)) and set(freed) == reserved and reserved, (prefix, sorted(reserved), sorted(freed))
        assert re.search(r"\b%s\(c\)" % release.split("::")[-1], callers), release


# ---- the hand-kept pairing of the uid map's validity and the tracers' slot table --------------------------------------
STALE_TABLES = ("tracers", "bonds.nt", "bends.nt", "areas.nt", "bodies")      # what keeps storage slots by uid


def marks_every_slot_table(helper_body):
    """The body of uid_slots_stale sets c->X.stale of every table of STALE_TABLES, and sets them true."""
    return (all(re.search(r"c->%s\.stale\s*=" % re.escape(s), helper_body) for s in STALE_TABLES)
            and bool(re.search(r"=\s*true;\s*$", helper_body)))


def _statements(code):
    """(statement, the statement after it) of a source without comments: split at ';', braces dropped, blanks folded."""
    parts = [" ".join(p.replace("{", " ").replace("}", " ").split()) for p in code.split(";")]
    return list(zip(parts, parts[1:] + [""]))


def unpaired_map_invalidations(csrc=CSRC):
    """Where csrc/*.hip clears uid.map_valid (outside uid_map_build, whose callers decide), or sets it true outside
    uid_map_ready (which rebuilds the map of uids that have not changed), without `uid_slots_stale(c)` as the next
    statement: [(file, statement)].  A site that forgets it lets later frames, bonds and bodies read rows through the
    storage indices of an older order, and past n after a removal (gpe_internal.h, TracerState::stale)."""
    bad, sites = [], 0
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        code = _code(path)
        for fn in ("uid_map_build", "uid_map_ready"):
            if re.search(r"^[\w:<> \*]*\b%s\([^{;]*\)\n\{" % fn, code, flags=re.M):
                code = code.replace(_body(code, fn), "")
        for stmt, after in _statements(code):
            if re.search(r"\bmap_valid\s*=\s*(false|true)$", stmt):
                sites += 1
                if not re.search(r"\buid_slots_stale\(c\)$", after):
                    bad.append((os.path.basename(path), stmt))
    return bad, sites


def test_every_map_invalidation_marks_the_tracers_slot_table_stale():
    """Every `map_valid = false` outside uid_map_build, and the one `map_valid = true` outside uid_map_ready
    (gpe_set_uids, whose map is that of new uids), is followed at once by `uid_slots_stale(c)`, which sets the stale flag
    of all five slot tables: the tracers', the bonds', the bends' and the areas' node tables and the bodies' members.
    Deleting any one of those lines from a copy of the sources makes unpaired_map_invalidations() name the site (tried
    with each in turn), and a copy of the helper with any one of the five flags dropped fails the check here (tried
    below, with each in turn)."""
    helper = re.search(r"inline void uid_slots_stale\(gpe_ctx \*c\) \{([^}]*)\}", _code(os.path.join(CSRC, "gpe_internal.h")))
    assert helper and marks_every_slot_table(helper.group(1)), helper
    for s in STALE_TABLES:
        without = helper.group(1).replace("c->%s.stale = " % s, "")
        assert without != helper.group(1) and not marks_every_slot_table(without), s
    assert not marks_every_slot_table(helper.group(1).replace("true", "false"))
    bad, sites = unpaired_map_invalidations()
    assert not bad, bad
    assert sites >= 8, sites                # (seven clear it, gpe_set_uids sets it; gpe_tracers_begin's own stale = true has no pair)


def test_the_pairing_check_notices_each_missing_line(tmp_path):
    """The check above on copies of csrc/ with one `uid_slots_stale(c)` line after a map_valid assignment removed:
    each copy fails, and names one site."""
    lines = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        src = open(path).read().split("\n")
        for i, line in enumerate(src):
            if re.search(r"uid_slots_stale\(c\);", line) and i and re.search(r"map_valid = (false|true);", src[i - 1]):
                lines[(path, i)] = src
    assert len(lines) >= 8, len(lines)
    for n, ((path, i), src) in enumerate(sorted(lines.items())):
        copy = tmp_path / ("csrc_%d" % n)
        copy.mkdir()
        for other in glob.glob(os.path.join(CSRC, "*.hip")):
            text = open(other).read() if other != path else "\n".join(src[:i] + src[i + 1:])
            (copy / os.path.basename(other)).write_text(text)
        bad, _ = unpaired_map_invalidations(str(copy))
        assert len(bad) == 1 and bad[0][0] == os.path.basename(path), (path, i, bad)
