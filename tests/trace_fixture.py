"""The file format of the trace fixtures (tests/golden/training_trace*.json).  A trace repeats itself -- the same launch for
every batch, the same event, bar or printed report in every mode of a case -- so a value that occurs more than once is stored
once: "rows" holds the distinct values in order of first appearance, and a case holds, under `key`, the list of the indices
of its rows (events or launches) and under every other field the index of that field's value.  load() gives back exactly what
dump() was handed."""
import json


def dump(path, cases, key):
    rows, index = [], {}

    def intern(value):
        s = json.dumps(value, separators=(',', ':'))
        if s not in index:
            index[s] = len(rows)
            rows.append(s)
        return index[s]

    packed = {name: {f: [intern(r) for r in v] if f == key else intern(v) for f, v in case.items()} for name, case in cases.items()}
    with open(path, "w") as f:
        f.write('{"rows": [\n' + ",\n".join(rows) + '\n],\n"cases": {\n'
                + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in packed.items()) + "\n}}\n")


def load(path, key):
    with open(path) as f:
        doc = json.load(f)
    rows = doc["rows"]
    return {name: {f: [rows[i] for i in v] if f == key else rows[v] for f, v in case.items()} for name, case in doc["cases"].items()}
