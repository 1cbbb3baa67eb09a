/*
 * ovl_digraph.c — the networkx DiGraph adjacency of the overlap graph, built in C (CPython extension
 * ovlgraph._digraph; host code, SURVEY.md §8f rank 2: edge materialisation).
 *
 * construct_overlap_graph_nx_k (overlapGraphs.py:55-60) adds one edge per (pair, copy of a, copy of b)
 * with networkx's add_edge: ~3 µs per edge in Python.  ovlgraph.overlapGraphs.assemble_graph_direct
 * expands the scored pairs into edge arrays (u, v node ids in insertion order, weight, end_position) and
 * this module builds exactly the dicts add_edge would have built:
 *   node[name] = {}                                   for every node in node order (overlapGraphs.py:25-28)
 *   d = {"weight": w, "end_position": e}              one attribute dict per edge,
 *   succ[names[u]][names[v]] = d; pred[names[v]][names[u]] = d   shared by both views, edges in global order
 * so successor, predecessor and edge-data views read identically to networkx's own construction.
 *
 *   build(names: list[str], u: int64[n], v: int64[n], weight: int32[n], end: int32[n][, shared: dict])
 *       -> (node, succ, pred)
 *
 * and, for remove_cycles_from_graph (overlapGraphs.py:106-130; the replay itself is ovl_remove_cycles in
 * ovl_graph.cpp), the two per-edge passes around the replay:
 *   csr(nodes, adj) -> (off, heads, weights)          the successor lists as CSR, in DFS visiting order
 *   remove_edges(succ, pred, nodes, tails, heads)      the replay's removals, in order, as remove_edge does
 *
 * Straight from the scored pair columns (ovlgraph.overlapGraphs.OverlapEdges; the lazy DiGraph), with no edge
 * arrays in between:
 *   overlap_csr(counts, a, b, score[, keep]) -> (off, heads, weights)
 *       the graph's successor lists as CSR: node first[r] + c is copy c of read r (overlapGraphs.py:25-28);
 *       its row is, for each kept pair p with a[p] == r in list order, the copies of b[p] (:55-60)
 *   build_overlap(names, counts, a, b, score, end[, keep[, alive[, shared]]]) -> (node, succ, pred)
 *       the dicts build() makes from the expanded edges, for the edges whose CSR index is alive only (the
 *       survivors of the cycle removal, in the reference's insertion order)
 */
#define PY_SSIZE_T_CLEAN
#include <Python.h>
#include <stdint.h>
#include <string.h>
#include <pthread.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

static int take(PyObject* obj, Py_buffer* view, Py_ssize_t itemsize, const char* what) {
    if (PyObject_GetBuffer(obj, view, PyBUF_C_CONTIGUOUS | PyBUF_FORMAT) != 0) return -1;
    if (view->itemsize != itemsize || view->len % itemsize != 0) {
        PyErr_Format(PyExc_TypeError, "%s: expected a contiguous array of %zd-byte integers", what, itemsize);
        PyBuffer_Release(view);
        return -1;
    }
    return 0;
}

/* Sized allocation: `count` elements, never a zero-byte request (an empty graph still gets valid pointers).
   NEW / NEW0 hold Python-side state (GIL held); RAW_NEW is for the buffers the helper threads read. */
static size_t nz(int64_t count) { return count > 0 ? (size_t)count : 1; }

static void* alloc_n(int64_t count, size_t size, int zeroed) {
    return zeroed ? PyMem_Calloc(nz(count), size) : PyMem_Malloc(nz(count) * size);
}
#define NEW(T, count) ((T*)alloc_n((int64_t)(count), sizeof(T), 0))
#define NEW0(T, count) ((T*)alloc_n((int64_t)(count), sizeof(T), 1))
#define RAW_NEW(T, count) ((T*)PyMem_RawMalloc(sizeof(T) * nz((int64_t)(count))))

static PyObject* key_weight(void) { return PyUnicode_InternFromString("weight"); }

/* Python ints for edge attributes: one object per distinct value in [kIntLo, kIntHi) (scores <= 10 * l and end
 * positions <= l for the reads of the benchmark configs), shared by every edge that carries it, instead of two
 * allocations per pair; values outside the range are created per pair. */
enum { kIntLo = -4096, kIntHi = 8192 };

static PyObject* int_of(PyObject** cache, long v) {
    if (v >= kIntLo && v < kIntHi) {
        PyObject** slot = &cache[v - kIntLo];
        if (!*slot) *slot = PyLong_FromLong(v);
        Py_XINCREF(*slot);
        return *slot;
    }
    return PyLong_FromLong(v);
}

/* The maker of the edges' attribute dicts {"weight": w, "end_position": e}, one per builder call.  A dict is a
   copy of the two-key template with its values set, cheaper than growing an empty dict by two inserts.  With
   `shared` (an instance __dict__ holding exactly the two keys, PEP 412 key-sharing) every copy shares the
   template's key table and owns only its values: 104 instead of 232 bytes per edge, and still an ordinary dict (a
   key added later converts that one dict).  On CPython 3.10 such a split-table template is copied with its values
   array, and the two values are written into that array directly (iw / ie: their slots in the template's key
   table) instead of two PyDict_SetItem lookups; any other dict takes the SetItem path. */
typedef struct {
    PyObject *kw, *ke;  /* the interned keys */
    PyObject* tmpl;
    Py_ssize_t iw, ie;  /* -1: no direct slots */
    PyObject** ints;    /* int_of's cache */
} Attrs;

static void attrs_free(Attrs* A) {
    if (A->ints)
        for (int i = 0; i < kIntHi - kIntLo; ++i) Py_XDECREF(A->ints[i]);
    PyMem_Free(A->ints);
    Py_XDECREF(A->tmpl);
    Py_XDECREF(A->kw);
    Py_XDECREF(A->ke);
    memset(A, 0, sizeof(*A));
}

/* `shared` is the template when it is a dict of exactly the two keys, else (NULL and None included) a fresh
   template is made.  0, or -1 with an exception set (attrs_free is safe either way). */
static int attrs_init(Attrs* A, PyObject* shared) {
    memset(A, 0, sizeof(*A));
    A->iw = A->ie = -1;
    A->kw = key_weight();
    A->ke = PyUnicode_InternFromString("end_position");
    A->ints = NEW0(PyObject*, kIntHi - kIntLo);
    if (!A->kw || !A->ke || !A->ints) {
        if (!PyErr_Occurred()) PyErr_NoMemory();
        return -1;
    }
    if (shared && PyDict_Check(shared) && PyDict_GET_SIZE(shared) == 2 && PyDict_Contains(shared, A->kw) == 1 &&
        PyDict_Contains(shared, A->ke) == 1) {
        A->tmpl = shared;
        Py_INCREF(A->tmpl);
    } else {
        A->tmpl = PyDict_New();
        if (!A->tmpl || PyDict_SetItem(A->tmpl, A->kw, Py_None) || PyDict_SetItem(A->tmpl, A->ke, Py_None)) return -1;
    }
#if PY_VERSION_HEX >= 0x030A0000 && PY_VERSION_HEX < 0x030B0000
    if (((PyDictObject*)A->tmpl)->ma_values != NULL) {
        Py_ssize_t pos = 0;
        PyObject *k, *v;
        while (PyDict_Next(A->tmpl, &pos, &k, &v)) {  /* (split table: pos - 1 is the slot in ma_values) */
            if (k == A->kw) A->iw = pos - 1;
            else if (k == A->ke) A->ie = pos - 1;
        }
        if (A->iw < 0 || A->ie < 0) A->iw = A->ie = -1;
    }
#endif
    return 0;
}

/* a new attribute dict holding the two ints (the caller keeps its references to them) */
static PyObject* attrs_dict(const Attrs* A, PyObject* wv, PyObject* ev) {
    PyObject* d = PyDict_Copy(A->tmpl);
    if (!d) return NULL;
#if PY_VERSION_HEX >= 0x030A0000 && PY_VERSION_HEX < 0x030B0000
    PyObject** vals = ((PyDictObject*)d)->ma_values;
    if (A->iw >= 0 && vals) {
        Py_INCREF(wv);
        Py_XSETREF(vals[A->iw], wv);
        Py_INCREF(ev);
        Py_XSETREF(vals[A->ie], ev);
        return d;
    }
#endif
    if (PyDict_SetItem(d, A->kw, wv) || PyDict_SetItem(d, A->ke, ev)) {
        Py_DECREF(d);
        return NULL;
    }
    return d;
}

/* a new attribute dict for one edge's score and end position */
static PyObject* attrs_edge(const Attrs* A, long score, long end) {
    PyObject* wv = int_of(A->ints, score);
    PyObject* ev = int_of(A->ints, end);
    PyObject* d = wv && ev ? attrs_dict(A, wv, ev) : NULL;
    Py_XDECREF(wv);
    Py_XDECREF(ev);
    return d;
}

/* The result's node-ordered top-level dicts, with every node's successor and predecessor dict created at its
   final size (no rehash while it fills); sin / pin borrow those per-node dicts from succ / pred. */
typedef struct {
    PyObject *node, *succ, *pred;
    PyObject **sin, **pin;
} Tops;

static void tops_free(Tops* T) {
    PyMem_Free(T->sin);
    PyMem_Free(T->pin);
    Py_XDECREF(T->node);
    Py_XDECREF(T->succ);
    Py_XDECREF(T->pred);
    memset(T, 0, sizeof(*T));
}

static int tops_make(Tops* T, PyObject* names, const int64_t* outdeg, const int64_t* indeg) {
    const Py_ssize_t n_nodes = PyList_GET_SIZE(names);
    memset(T, 0, sizeof(*T));
    T->node = PyDict_New();
    T->succ = PyDict_New();
    T->pred = PyDict_New();
    T->sin = NEW(PyObject*, n_nodes);
    T->pin = NEW(PyObject*, n_nodes);
    if (!T->node || !T->succ || !T->pred || !T->sin || !T->pin) {
        if (!PyErr_Occurred()) PyErr_NoMemory();
        return -1;
    }
    for (Py_ssize_t i = 0; i < n_nodes; ++i) {
        PyObject* name = PyList_GET_ITEM(names, i);
        PyObject* x = PyDict_New();
        PyObject* sd = _PyDict_NewPresized(outdeg[i]);
        PyObject* pd = _PyDict_NewPresized(indeg[i]);
        const int bad = !x || !sd || !pd || PyDict_SetItem(T->node, name, x) || PyDict_SetItem(T->succ, name, sd) ||
                        PyDict_SetItem(T->pred, name, pd);
        Py_XDECREF(x);
        Py_XDECREF(sd);
        Py_XDECREF(pd);
        if (bad) return -1;
        T->sin[i] = sd;
        T->pin[i] = pd;
    }
    return 0;
}

static PyObject* build_impl(PyObject* self, PyObject* args) {
    (void)self;
    PyObject *names, *ou, *ov, *ow, *oe, *shared = NULL;
    if (!PyArg_ParseTuple(args, "O!OOOO|O!", &PyList_Type, &names, &ou, &ov, &ow, &oe, &PyDict_Type, &shared))
        return NULL;
    Py_buffer bu = {0}, bv = {0}, bw = {0}, be = {0};
    PyObject* out = NULL;
    Tops T;
    memset(&T, 0, sizeof(T));
    Attrs A;
    memset(&A, 0, sizeof(A));
    int64_t* deg = NULL;
    if (take(ou, &bu, 8, "u") || take(ov, &bv, 8, "v") || take(ow, &bw, 4, "weight") || take(oe, &be, 4, "end"))
        goto done;
    const Py_ssize_t n_nodes = PyList_GET_SIZE(names);
    const Py_ssize_t n = bu.len / 8;
    const int64_t* u = (const int64_t*)bu.buf;
    const int64_t* v = (const int64_t*)bv.buf;
    const int32_t* w = (const int32_t*)bw.buf;
    const int32_t* e = (const int32_t*)be.buf;
    if (bv.len / 8 != n || bw.len / 4 != n || be.len / 4 != n) {
        PyErr_SetString(PyExc_ValueError, "u, v, weight and end must have the same length");
        goto done;
    }
    /* out- and in-degrees first: the dicts' final sizes */
    deg = NEW0(int64_t, 2 * n_nodes);
    if (!deg) { PyErr_NoMemory(); goto done; }
    for (Py_ssize_t k = 0; k < n; ++k) {
        if (u[k] < 0 || u[k] >= n_nodes || v[k] < 0 || v[k] >= n_nodes) {
            PyErr_Format(PyExc_IndexError, "edge %zd: node id outside [0, %zd)", k, n_nodes);
            goto done;
        }
        ++deg[u[k]];
        ++deg[n_nodes + v[k]];
    }
    if (tops_make(&T, names, deg, deg + n_nodes) || attrs_init(&A, shared)) goto done;
    for (Py_ssize_t k = 0; k < n; ++k) {
        PyObject* d = attrs_edge(&A, w[k], e[k]);
        const int bad = !d || PyDict_SetItem(T.sin[u[k]], PyList_GET_ITEM(names, v[k]), d) ||
                        PyDict_SetItem(T.pin[v[k]], PyList_GET_ITEM(names, u[k]), d);
        Py_XDECREF(d);
        if (bad) goto done;
    }
    out = PyTuple_Pack(3, T.node, T.succ, T.pred);
done:
    PyMem_Free(deg);
    tops_free(&T);
    attrs_free(&A);
    if (bu.obj) PyBuffer_Release(&bu);
    if (bv.obj) PyBuffer_Release(&bv);
    if (bw.obj) PyBuffer_Release(&bw);
    if (be.obj) PyBuffer_Release(&be);
    return out;
}

/* The integer value of an edge's "weight" (an int, not a bool, or an instance of `more`, e.g. numpy.integer),
 * as remove_cycles_from_graph requires; -1 with an exception set on a missing or non-integer weight. */
static int weight_of(PyObject* attrs, PyObject* kw, PyObject* more, long long* out) {
    PyObject* w = PyDict_Check(attrs) ? PyDict_GetItemWithError(attrs, kw) : NULL;
    if (!w) {
        if (!PyErr_Occurred()) PyErr_SetObject(PyExc_KeyError, kw);
        return -1;
    }
    if (PyBool_Check(w)) goto bad;
    if (PyLong_Check(w)) {
        *out = PyLong_AsLongLong(w);
        return (*out == -1 && PyErr_Occurred()) ? -1 : 0;
    }
    if (more && PyObject_IsInstance(w, more) == 1) {
        PyObject* iv = PyNumber_Index(w);
        if (!iv) goto bad;
        *out = PyLong_AsLongLong(iv);
        Py_DECREF(iv);
        return (*out == -1 && PyErr_Occurred()) ? -1 : 0;
    }
bad:
    PyErr_Clear();
    PyErr_SetString(PyExc_TypeError, "remove_cycles_from_graph needs an integer 'weight' on every edge");
    return -1;
}

/* csr(nodes, adj[, more]) -> (off, heads, weights): the graph's successor lists as CSR in node order and, per node,
 * in adjacency order (the order networkx's DFS visits them): off int64[n+1], heads int32[E] (node indices),
 * weights int64[E], as bytearrays; None when a row is not exactly a dict (the caller's Python passes then).
 * One pass in C instead of three Python generators over 10^6-10^7 edges. */
static PyObject* csr(PyObject* self, PyObject* args) {
    (void)self;
    PyObject *nodes, *adj, *more = NULL;
    if (!PyArg_ParseTuple(args, "O!O!|O", &PyList_Type, &nodes, &PyDict_Type, &adj, &more)) return NULL;
    const Py_ssize_t n_nodes = PyList_GET_SIZE(nodes);
    PyObject *index = NULL, *boff = NULL, *bheads = NULL, *bw = NULL, *kw = NULL, *out = NULL;
    PyObject** rows = NEW(PyObject*, n_nodes);
    index = PyDict_New();
    kw = key_weight();
    boff = PyByteArray_FromStringAndSize(NULL, (Py_ssize_t)(8 * (n_nodes + 1)));
    if (!rows || !index || !kw || !boff) { if (!PyErr_Occurred()) PyErr_NoMemory(); goto done; }
    int64_t* off = (int64_t*)PyByteArray_AS_STRING(boff);
    off[0] = 0;
    for (Py_ssize_t i = 0; i < n_nodes; ++i) {
        PyObject* name = PyList_GET_ITEM(nodes, i);
        PyObject* iv = PyLong_FromSsize_t(i);
        if (!iv || PyDict_SetItem(index, name, iv)) { Py_XDECREF(iv); goto done; }
        Py_DECREF(iv);
        PyObject* row = PyDict_GetItemWithError(adj, name);
        if (!row) { if (!PyErr_Occurred()) PyErr_SetObject(PyExc_KeyError, name); goto done; }
        if (!PyDict_CheckExact(row)) {  /* a dict subclass may iterate in another order: caller's fallback */
            out = Py_None;
            Py_INCREF(out);
            goto done;
        }
        rows[i] = row;  /* borrowed: adj holds it */
        off[i + 1] = off[i] + PyDict_GET_SIZE(row);
    }
    const int64_t n_edges = off[n_nodes];
    bheads = PyByteArray_FromStringAndSize(NULL, (Py_ssize_t)(4 * nz(n_edges)));
    bw = PyByteArray_FromStringAndSize(NULL, (Py_ssize_t)(8 * nz(n_edges)));
    if (!bheads || !bw) goto done;
    int32_t* heads = (int32_t*)PyByteArray_AS_STRING(bheads);
    long long* wts = (long long*)PyByteArray_AS_STRING(bw);
    int64_t e = 0;
    for (Py_ssize_t i = 0; i < n_nodes; ++i) {
        Py_ssize_t pos = 0;
        PyObject *v, *attrs;
        while (PyDict_Next(rows[i], &pos, &v, &attrs)) {
            PyObject* iv = PyDict_GetItemWithError(index, v);
            if (!iv) { if (!PyErr_Occurred()) PyErr_SetObject(PyExc_KeyError, v); goto done; }
            heads[e] = (int32_t)PyLong_AsLong(iv);
            if (weight_of(attrs, kw, more, &wts[e]) != 0) goto done;
            ++e;
        }
    }
    out = PyTuple_Pack(3, boff, bheads, bw);
done:
    PyMem_Free(rows);
    Py_XDECREF(index);
    Py_XDECREF(kw);
    Py_XDECREF(boff);
    Py_XDECREF(bheads);
    Py_XDECREF(bw);
    return out;
}

/* remove_edges(succ, pred, nodes, tails: int64[k], heads: int64[k]): for each i in order,
 * del succ[nodes[tails[i]]][nodes[heads[i]]]; del pred[nodes[heads[i]]][nodes[tails[i]]] -- networkx's
 * DiGraph.remove_edge without its per-call cache clear (the caller clears once).  KeyError if an edge is
 * absent (edges before it stay removed, as with a loop of remove_edge). */
static PyObject* remove_edges(PyObject* self, PyObject* args) {
    (void)self;
    PyObject *succ, *pred, *nodes, *ot, *oh;
    if (!PyArg_ParseTuple(args, "O!O!O!OO", &PyDict_Type, &succ, &PyDict_Type, &pred, &PyList_Type, &nodes, &ot, &oh))
        return NULL;
    Py_buffer bt, bh;
    if (take(ot, &bt, 8, "tails") != 0) return NULL;
    if (take(oh, &bh, 8, "heads") != 0) { PyBuffer_Release(&bt); return NULL; }
    PyObject* ret = NULL;
    const Py_ssize_t n_nodes = PyList_GET_SIZE(nodes);
    const Py_ssize_t k = bt.len / 8;
    const int64_t* t = (const int64_t*)bt.buf;
    const int64_t* h = (const int64_t*)bh.buf;
    if (bh.len / 8 != k) { PyErr_SetString(PyExc_ValueError, "tails and heads must have the same length"); goto done; }
    for (Py_ssize_t i = 0; i < k; ++i) {
        if (t[i] < 0 || t[i] >= n_nodes || h[i] < 0 || h[i] >= n_nodes) {
            PyErr_Format(PyExc_IndexError, "edge %zd: node index outside [0, %zd)", i, n_nodes);
            goto done;
        }
        PyObject* u = PyList_GET_ITEM(nodes, t[i]);
        PyObject* v = PyList_GET_ITEM(nodes, h[i]);
        PyObject* su = PyDict_GetItemWithError(succ, u);
        PyObject* pv = su ? PyDict_GetItemWithError(pred, v) : NULL;
        if (!su || !pv || !PyDict_Check(su) || !PyDict_Check(pv) || PyDict_DelItem(su, v) || PyDict_DelItem(pv, u)) {
            if (!PyErr_Occurred()) PyErr_Format(PyExc_KeyError, "edge %zd is not in the graph", i);
            goto done;
        }
    }
    ret = Py_None;
    Py_INCREF(ret);
done:
    PyBuffer_Release(&bt);
    PyBuffer_Release(&bh);
    return ret;
}

/* The pair columns of overlap_csr and the two column builders: counts (int32, one per read); a, b, score and end
   (int32, one per pair; overlap_csr takes no end); the optional keep mask (uint8 per pair, or None). */
typedef struct {
    Py_buffer bc, ba, bb, bs, be, bk;
    Py_ssize_t R, P;  /* reads, pairs */
    const int32_t *counts, *a, *b, *sc, *en;
    const uint8_t* keep;  /* NULL: every pair is kept */
} PairCols;

static void pairs_release(PairCols* Q) {
    Py_buffer* const all[] = {&Q->bc, &Q->ba, &Q->bb, &Q->bs, &Q->be, &Q->bk};
    for (int i = 0; i < 6; ++i)
        if (all[i]->obj) PyBuffer_Release(all[i]);
}

/* oe NULL: no end column.  0, or -1 with an exception set; pairs_release is due either way. */
static int pairs_take(PairCols* Q, PyObject* oc, PyObject* oa, PyObject* ob, PyObject* os, PyObject* oe,
                      PyObject* ok) {
    memset(Q, 0, sizeof(*Q));
    if (take(oc, &Q->bc, 4, "counts") || take(oa, &Q->ba, 4, "a") || take(ob, &Q->bb, 4, "b")) return -1;
    if (Q->ba.len != Q->bb.len) { PyErr_SetString(PyExc_ValueError, "a and b must have the same length"); return -1; }
    Q->R = Q->bc.len / 4;
    Q->P = Q->ba.len / 4;
    if (ok && ok != Py_None) {
        if (take(ok, &Q->bk, 1, "keep")) return -1;
        if (Q->bk.len != Q->P) { PyErr_SetString(PyExc_ValueError, "keep must have one entry per pair"); return -1; }
        Q->keep = (const uint8_t*)Q->bk.buf;
    }
    if (take(os, &Q->bs, 4, "score") || (oe && take(oe, &Q->be, 4, "end"))) return -1;
    if (Q->bs.len != Q->ba.len || (oe && Q->be.len != Q->ba.len)) {
        PyErr_SetString(PyExc_ValueError, oe ? "score and end must have one entry per pair"
                                             : "score must have one entry per pair");
        return -1;
    }
    Q->counts = (const int32_t*)Q->bc.buf;
    Q->a = (const int32_t*)Q->ba.buf;
    Q->b = (const int32_t*)Q->bb.buf;
    Q->sc = (const int32_t*)Q->bs.buf;
    Q->en = (const int32_t*)Q->be.buf;
    return 0;
}

/* The CSR layout of the overlap graph from the pair columns.  Pairs are grouped by read a (counting sort,
 * list order kept inside a group); row u = first[r] + c of read r has len rowlen[r] = sum of counts[b[p]] over
 * the group, the same for every copy c; pair p's edges sit at off[u] + pstart[p] + cb.  Returns 0, or -1 with
 * an exception set. */
typedef struct {
    Py_ssize_t R, P, N;
    int64_t E;
    int64_t* first;   /* R + 1 */
    int64_t* goff;    /* R + 1: group offsets into plist */
    int64_t* plist;   /* kept pairs grouped by a */
    int64_t* rowlen;  /* R */
    int64_t* pstart;  /* P (kept pairs) */
    int64_t* off;     /* N + 1 */
} Layout;

static void layout_free(Layout* L) {
    PyMem_Free(L->first);
    PyMem_Free(L->goff);
    PyMem_Free(L->plist);
    PyMem_Free(L->rowlen);
    PyMem_Free(L->pstart);
    PyMem_Free(L->off);
    memset(L, 0, sizeof(*L));
}

static int layout(Layout* L, const PairCols* Q) {
    const int32_t *counts = Q->counts, *a = Q->a, *b = Q->b;
    const uint8_t* keep = Q->keep;
    const Py_ssize_t R = Q->R, P = Q->P;
    memset(L, 0, sizeof(*L));
    L->R = R;
    L->P = P;
    L->first = NEW0(int64_t, R + 1);
    L->goff = NEW0(int64_t, R + 1);
    L->plist = NEW(int64_t, P);
    L->rowlen = NEW0(int64_t, R);
    L->pstart = NEW0(int64_t, P);
    if (!L->first || !L->goff || !L->plist || !L->rowlen || !L->pstart) { PyErr_NoMemory(); return -1; }
    for (Py_ssize_t r = 0; r < R; ++r) {
        if (counts[r] < 0) { PyErr_SetString(PyExc_ValueError, "negative copy count"); return -1; }
        L->first[r + 1] = L->first[r] + counts[r];
    }
    L->N = (Py_ssize_t)L->first[R];
    for (Py_ssize_t p = 0; p < P; ++p) {
        if (a[p] < 0 || a[p] >= R || b[p] < 0 || b[p] >= R) {
            PyErr_Format(PyExc_IndexError, "pair %zd: read index outside [0, %zd)", p, R);
            return -1;
        }
        if (keep && !keep[p]) continue;
        ++L->goff[a[p] + 1];
    }
    for (Py_ssize_t r = 0; r < R; ++r) L->goff[r + 1] += L->goff[r];
    int64_t* fill = NEW(int64_t, R);
    if (!fill) { PyErr_NoMemory(); return -1; }
    memcpy(fill, L->goff, sizeof(int64_t) * (size_t)R);
    for (Py_ssize_t p = 0; p < P; ++p) {
        if (keep && !keep[p]) continue;
        const int32_t r = a[p];
        L->plist[fill[r]++] = p;
        L->pstart[p] = L->rowlen[r];
        L->rowlen[r] += counts[b[p]];
    }
    PyMem_Free(fill);
    L->off = NEW(int64_t, L->N + 1);
    if (!L->off) { PyErr_NoMemory(); return -1; }
    L->off[0] = 0;
    for (Py_ssize_t r = 0; r < R; ++r)
        for (int64_t u = L->first[r]; u < L->first[r + 1]; ++u) L->off[u + 1] = L->off[u] + L->rowlen[r];
    L->E = L->off[L->N];
    return 0;
}

static PyObject* overlap_csr(PyObject* self, PyObject* args) {
    (void)self;
    PyObject *oc, *oa, *ob, *os, *ok = NULL;
    if (!PyArg_ParseTuple(args, "OOOO|O", &oc, &oa, &ob, &os, &ok)) return NULL;
    PairCols Q;
    Layout L;
    memset(&L, 0, sizeof(L));
    PyObject *boff = NULL, *bh = NULL, *bw = NULL, *out = NULL;
    if (pairs_take(&Q, oc, oa, ob, os, NULL, ok) || layout(&L, &Q)) goto done;
    boff = PyByteArray_FromStringAndSize((const char*)L.off, (Py_ssize_t)(8 * ((size_t)L.N + 1)));
    bh = PyByteArray_FromStringAndSize(NULL, (Py_ssize_t)(4 * nz(L.E)));
    bw = PyByteArray_FromStringAndSize(NULL, (Py_ssize_t)(8 * nz(L.E)));
    if (!boff || !bh || !bw) goto done;
    int32_t* heads = (int32_t*)PyByteArray_AS_STRING(bh);
    int64_t* wts = (int64_t*)PyByteArray_AS_STRING(bw);
    for (Py_ssize_t r = 0; r < L.R; ++r) {
        if (L.first[r + 1] == L.first[r]) continue;
        const int64_t u0 = L.first[r];
        int64_t e = L.off[u0];
        for (int64_t g = L.goff[r]; g < L.goff[r + 1]; ++g) {
            const int64_t p = L.plist[g];
            const int64_t v0 = L.first[Q.b[p]];
            for (int32_t cb = 0; cb < Q.counts[Q.b[p]]; ++cb, ++e) {
                heads[e] = (int32_t)(v0 + cb);
                wts[e] = Q.sc[p];
            }
        }
        /* every other copy of read r has the same row */
        for (int64_t u = u0 + 1; u < L.first[r + 1]; ++u) {
            memcpy(heads + L.off[u], heads + L.off[u0], sizeof(int32_t) * (size_t)L.rowlen[r]);
            memcpy(wts + L.off[u], wts + L.off[u0], sizeof(int64_t) * (size_t)L.rowlen[r]);
        }
    }
    out = PyTuple_Pack(3, boff, bh, bw);
done:
    layout_free(&L);
    pairs_release(&Q);
    Py_XDECREF(boff);
    Py_XDECREF(bh);
    Py_XDECREF(bw);
    return out;
}

static PyObject* build_overlap_impl(PyObject* self, PyObject* args) {
    (void)self;
    PyObject *names, *oc, *oa, *ob, *os, *oe, *ok = NULL, *oalive = NULL, *shared = NULL;
    if (!PyArg_ParseTuple(args, "O!OOOOO|OOO!", &PyList_Type, &names, &oc, &oa, &ob, &os, &oe, &ok, &oalive,
                          &PyDict_Type, &shared))
        return NULL;
    PairCols Q;
    memset(&Q, 0, sizeof(Q));
    Py_buffer bal;
    memset(&bal, 0, sizeof(bal));
    Layout L;
    memset(&L, 0, sizeof(L));
    Tops T;
    memset(&T, 0, sizeof(T));
    Attrs A;
    memset(&A, 0, sizeof(A));
    PyObject* out = NULL;
    int64_t *dout = NULL, *din = NULL;
    const uint8_t* alive = NULL;
    if (pairs_take(&Q, oc, oa, ob, os, oe, ok) || layout(&L, &Q)) goto done;
    if (PyList_GET_SIZE(names) != L.N) {
        PyErr_Format(PyExc_ValueError, "%zd names for %zd nodes", PyList_GET_SIZE(names), L.N);
        goto done;
    }
    if (oalive && oalive != Py_None) {
        if (take(oalive, &bal, 1, "alive")) goto done;
        if (bal.len != L.E) { PyErr_SetString(PyExc_ValueError, "alive must have one entry per edge"); goto done; }
        alive = (const uint8_t*)bal.buf;
    }
    /* live degrees: every dict is created at its final size */
    dout = NEW0(int64_t, L.N);
    din = NEW0(int64_t, L.N);
    if (!dout || !din) { PyErr_NoMemory(); goto done; }
    for (Py_ssize_t g = 0; g < (Py_ssize_t)L.goff[L.R]; ++g) {
        const int64_t p = L.plist[g];
        for (int64_t u = L.first[Q.a[p]]; u < L.first[Q.a[p] + 1]; ++u) {
            const int64_t e0 = L.off[u] + L.pstart[p];
            for (int32_t cb = 0; cb < Q.counts[Q.b[p]]; ++cb)
                if (!alive || alive[e0 + cb]) {
                    ++dout[u];
                    ++din[L.first[Q.b[p]] + cb];
                }
        }
    }
    if (tops_make(&T, names, dout, din) || attrs_init(&A, shared)) goto done;
    /* one pass over the edges in global insertion order (pair, copy of a, copy of b: overlapGraphs.py:43-60):
       each attribute dict goes into its tail's successor dict and its head's predecessor dict while it is
       still in cache.  A node's successors arrive in that order too, which is its CSR row order.  The two ints
       are made once per pair and shared by all its copies. */
    for (Py_ssize_t p = 0; p < L.P; ++p) {
        if (Q.keep && !Q.keep[p]) continue;
        PyObject *wv = NULL, *ev = NULL;
        int bad = 0;
        const int64_t vb = L.first[Q.b[p]];
        for (int64_t u = L.first[Q.a[p]]; u < L.first[Q.a[p] + 1] && !bad; ++u) {
            const int64_t e0 = L.off[u] + L.pstart[p];
            PyObject* un = PyList_GET_ITEM(names, u);
            for (int32_t cb = 0; cb < Q.counts[Q.b[p]] && !bad; ++cb) {
                if (alive && !alive[e0 + cb]) continue;
                if (!wv) {
                    wv = int_of(A.ints, Q.sc[p]);
                    ev = int_of(A.ints, Q.en[p]);
                }
                PyObject* d = wv && ev ? attrs_dict(&A, wv, ev) : NULL;
                bad = !d || PyDict_SetItem(T.sin[u], PyList_GET_ITEM(names, vb + cb), d) ||
                      PyDict_SetItem(T.pin[vb + cb], un, d);
                Py_XDECREF(d);
            }
        }
        Py_XDECREF(wv);
        Py_XDECREF(ev);
        if (bad) goto done;
    }
    out = PyTuple_Pack(3, T.node, T.succ, T.pred);
done:
    layout_free(&L);
    pairs_release(&Q);
    if (bal.obj) PyBuffer_Release(&bal);
    PyMem_Free(dout);
    PyMem_Free(din);
    tops_free(&T);
    attrs_free(&A);
    return out;
}

/* Out-edges that no removal can touch: remove_cycles_from_graph removes an edge only as the weakest of a cycle it
   lies on, so a node in a strongly connected component of its own (and without a live self-loop) never loses an
   out-edge again -- removals only delete edges, so components only split.  That holds for far more nodes, and far
   sooner, than the replay's own final set (nodes that can reach no cycle, or whose start's walk is over: at the
   target point 60 % of the nodes only at the end).  The helper recomputes the components of the live graph (Tarjan,
   iterative) pass after pass while the replay runs and publishes every node newly alone in its component.  It reads
   `alive` while the replay clears entries, so a pass sees a superset of the live edges; the components of a
   supergraph contain the true ones, so a node alone in a pass's graph is alone in the true graph too.  Edges into
   published nodes are skipped in later passes (such a node is on no cycle). */
typedef struct {
    const int64_t* off;
    const int32_t* heads;
    const uint8_t* alive;
    int32_t n;
    const int* stop;       /* the replay's finished flag */
    int* gate;             /* set after the first pass (else already set) */
    int32_t* nodes;        /* published nodes [0, n_pub) (release-ordered count) */
    int64_t n_pub;
    int passes;
    int ok;
} SccJob;

static void* scc_main(void* arg) {
    SccJob* j = (SccJob*)arg;
    const int32_t N = j->n;
    int32_t* index = (int32_t*)malloc(sizeof(int32_t) * nz(N));
    int32_t* low = (int32_t*)malloc(sizeof(int32_t) * nz(N));
    int32_t* stk = (int32_t*)malloc(sizeof(int32_t) * nz(N));
    int32_t* cv = (int32_t*)malloc(sizeof(int32_t) * nz(N));  /* call stack: node */
    int64_t* cp = (int64_t*)malloc(sizeof(int64_t) * nz(N));  /* call stack: next edge */
    uint8_t* on = (uint8_t*)malloc(nz(N));
    uint8_t* alone = (uint8_t*)calloc(nz(N), 1);
    if (!index || !low || !stk || !cv || !cp || !on || !alone) goto out;
    j->ok = 1;
    while (!__atomic_load_n(j->stop, __ATOMIC_ACQUIRE)) {
        for (int32_t v = 0; v < N; ++v) index[v] = -1;
        memset(on, 0, (size_t)N);
        int32_t idx = 0, sp = 0;
        int64_t pub = j->n_pub;
        const int64_t pub0 = pub;
        for (int32_t r = 0; r < N && !__atomic_load_n(j->stop, __ATOMIC_RELAXED); ++r) {
            if (index[r] >= 0 || alone[r]) continue;
            int32_t depth = 0;
            cv[0] = r;
            cp[0] = j->off[r];
            index[r] = low[r] = idx++;
            stk[sp++] = r;
            on[r] = 1;
            while (depth >= 0) {
                const int32_t v = cv[depth];
                const int64_t end = j->off[v + 1];
                int64_t e = cp[depth];
                int descended = 0;
                for (; e < end; ++e) {
                    if (!__atomic_load_n(&j->alive[e], __ATOMIC_ACQUIRE)) continue;
                    const int32_t w = j->heads[e];
                    if (alone[w]) continue;
                    if (index[w] < 0) {
                        cp[depth] = e + 1;
                        ++depth;
                        cv[depth] = w;
                        cp[depth] = j->off[w];
                        index[w] = low[w] = idx++;
                        stk[sp++] = w;
                        on[w] = 1;
                        descended = 1;
                        break;
                    }
                    if (on[w] && index[w] < low[v]) low[v] = index[w];
                }
                if (descended) continue;
                /* v is done: the root of a component? */
                if (low[v] == index[v]) {
                    if (stk[sp - 1] == v) {
                        /* a component of one: alone unless a live self-loop */
                        int loop = 0;
                        for (int64_t f = j->off[v]; f < end && !loop; ++f)
                            loop = j->heads[f] == v && __atomic_load_n(&j->alive[f], __ATOMIC_ACQUIRE);
                        if (!loop) {
                            alone[v] = 1;
                            j->nodes[pub++] = v;
                            __atomic_store_n(&j->n_pub, pub, __ATOMIC_RELEASE);
                        }
                    }
                    int32_t x;
                    do {
                        x = stk[--sp];
                        on[x] = 0;
                    } while (x != v);
                }
                --depth;
                if (depth >= 0 && low[v] < low[cv[depth]]) low[cv[depth]] = low[v];
            }
        }
        ++j->passes;
        __atomic_store_n(j->gate, 1, __ATOMIC_RELEASE);
        if (j->n_pub == pub0) {  /* nothing new: let the replay remove more before the next pass */
            struct timespec ts = {0, 300000};
            nanosleep(&ts, NULL);
        }
    }
out:
    __atomic_store_n(j->gate, 1, __ATOMIC_RELEASE);
    free(index);
    free(low);
    free(stk);
    free(cv);
    free(cp);
    free(on);
    free(alone);
    return NULL;
}

/* OVL_TRACE_STREAM=1 (diagnostics): one stderr line per build_overlap_stream with the millisecond offsets of its
   phases (s setup done, r replay finished as seen here, with the share of the nodes whose rows were built by
   then, b dicts built, t top-level dicts), the replay thread's own time and the CPUs both threads ran on */
static double now_ms(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

typedef int (*replay_stream_fn)(const int64_t*, const int32_t*, const int64_t*, int32_t, int64_t*, int64_t*,
                                uint8_t*, int32_t*, int64_t*);
typedef struct {
    replay_stream_fn fn;
    const int64_t* off;
    const int32_t* heads;
    const int64_t* w;
    int32_t n;
    int64_t* removed;
    int64_t n_removed;
    uint8_t* alive;
    int32_t* final_nodes;
    int64_t n_final;
    int rc;
    int finished;
    int gate;       /* the replay starts once this is non-zero (OVL_STREAM_SCC=2: after the helper's first pass) */
    int cpu_main;   /* the calling thread's CPU when the replay started */
    int cpu_start, cpu_end;
    double ms;      /* the replay's own duration */
} ReplayJob;

static void* replay_main(void* arg) {
    ReplayJob* j = (ReplayJob*)arg;
    while (!__atomic_load_n(&j->gate, __ATOMIC_ACQUIRE)) sched_yield();
    j->cpu_start = sched_getcpu();
    const double t0 = now_ms();
    j->rc = j->fn(j->off, j->heads, j->w, j->n, j->removed, &j->n_removed, j->alive, j->final_nodes, &j->n_final);
    j->ms = now_ms() - t0;
    j->cpu_end = sched_getcpu();
    __atomic_store_n(&j->finished, 1, __ATOMIC_RELEASE);
    return NULL;
}

/* build_overlap_stream(names, counts, a, b, score, end, keep, shared, replay_fn, off, heads, weights)
 *     -> (node, succ, pred, removed, n_removed)
 * remove_cycles_from_graph on a graph that is still columns, with the replay and the dicts overlapped: the replay
 * (replay_fn = the address of libovl's ovl_remove_cycles_stream) runs on a second thread over the CSR (off,
 * heads, weights: OverlapEdges.csr()), and this thread builds each node's successor dict as soon as the replay
 * publishes that node's out-edges as final (they can no longer be removed), with the edges' attribute dicts, and
 * each node's predecessor dict as soon as every tail of its in-edges is final: its in-edges in global insertion
 * order (pairs with b = its read in list order, then the copies of a: overlapGraphs.py:43-60); then the
 * node-ordered top-level dicts.  The result is build_overlap's for the alive mask of the replay; removed holds
 * the replay's removed CSR indices (int64) in removal order. */
/* Everything one build_overlap_stream call owns.  The phases below fill it in, in the order the entry function
   lists them, each returning 0, or -1 with an exception set; stream_free releases it on every exit. */
typedef struct {
    PyObject* names;          /* (borrowed) */
    PairCols Q;
    Py_buffer off, heads, w;  /* the caller's CSR */
    int64_t N, E;             /* its nodes and edges: the layout's too, once stream_layout has checked them */
    Layout L;
    Attrs A;
    PyObject* gc_collect;
    /* the replay and the component helper: job and scc are theirs to read and write while they run */
    ReplayJob job;
    SccJob scc;
    pthread_t th, scc_th;
    int started, scc_started;
    int scc_on;  /* OVL_STREAM_SCC (tests, A/B): 0 rows only as the replay publishes them (no component helper);
                    2 the replay waits for the helper's first pass (every node alone in the whole graph's
                    components goes first) */
    /* in-edges in insertion order: each node's read; the kept pairs grouped by b (list order within a group); a
       node's in-edges, live or not (its predecessor dict's presize), and out-edges (its row's) */
    int64_t *rread, *bgoff, *blist, *pending, *outdeg;
    PyObject **rows, **pin;  /* per node: its successor and predecessor dict (references; NULL: not made yet) */
    PyObject** dptr;         /* per edge: its attribute dict once inserted, for the head's predecessor cursor */
    PyObject** spec;         /* per edge: its attribute dict made ahead of its row (spec_advance), or NULL */
    int own_refs;            /* dptr's entries are references (only when some (a, b) pair is listed twice) */
    uint8_t* dec;            /* per edge: its fate is known (its tail's row has passed it) */
    uint8_t* pubd;           /* per node: published (on no cycle) */
    int64_t *pg, *pt;        /* predecessor cursor: pair group (-1: complete) and tail copy */
    int64_t* rg;             /* row cursor: pair group (-1: complete) */
    int32_t* rc;             /*             copy of b */
    int64_t* openl;          /* the nodes whose rows are open */
    int64_t spec_u, reap_e;  /* spec_advance's next node, spec_reap's next edge */
    PyObject *node, *succ, *pred;
    /* counts, for the final check and the trace line: complete predecessor dicts and rows, decided edges, live
       edges inserted, attribute dicts made ahead and of those inserted; nodes the replay published, nodes the helper
       published first, sweeps, collections */
    int64_t n_pred, n_rows, n_dec, n_ins, n_spec, n_spec_used, k_done, n_from_scc, n_sweeps;
    int n_gc;
    int trace;  /* OVL_TRACE_STREAM */
    double t0, t_setup, t_replay, t_built, t_tops, t_gc;
    int64_t k_at_replay, dec_at_replay, ins_at_replay;
} StreamBuild;

/* A node's predecessor dict, built as a prefix of its in-edges in insertion order (kept pairs with b == its read in
   list order, then the copies of a): the cursor (pg, pt: pair group and tail copy) advances while the next in-edge's
   fate is known (its tail's successor row has passed it: dec), inserting the live ones. */
static int pred_advance(StreamBuild* S, int64_t v) {
    int64_t g = S->pg[v];
    if (g < 0) return 0;
    const Py_ssize_t rv = (Py_ssize_t)S->rread[v];
    const int64_t gend = S->bgoff[rv + 1];
    const int64_t cv = v - S->L.first[rv];
    int64_t t = S->pt[v];
    while (g < gend) {
        const int64_t q = S->blist[g];
        const int64_t tend = S->L.first[S->Q.a[q] + 1];
        for (; t < tend; ++t) {
            const int64_t e = S->L.off[t] + S->L.pstart[q] + cv;
            if (!S->dec[e]) {
                S->pg[v] = g;
                S->pt[v] = t;
                return 0;
            }
            PyObject* d = S->dptr[e];
            if (d) {
                if (!S->pin[v] && !(S->pin[v] = _PyDict_NewPresized(S->pending[v]))) return -1;
                if (PyDict_SetItem(S->pin[v], PyList_GET_ITEM(S->names, t), d)) return -1;
            }
        }
        if (++g < gend) t = S->L.first[S->Q.a[S->blist[g]]];
    }
    if (!S->pin[v] && !(S->pin[v] = PyDict_New())) return -1;
    S->pg[v] = -1;
    ++S->n_pred;
    return 0;
}

/* A node's successor dict, built the same way as a prefix of its out-edges in row order (kept pairs with a == its
   read in list order, then the copies of b): an out-edge's fate is known once it is removed (alive 0: removals are
   final), once its head is on no cycle (published by the replay or the component helper: no cycle can hold the
   edge, so it is never removed), or once the tail itself is published (all its out-edges final).  Each edge passed
   is marked decided and lets its head's predecessor dict advance.  `all`: u is published (every edge decided).
   1 if the row moved, 0 if not, -1 on error. */
static int row_advance(StreamBuild* S, int64_t u, int all) {
    int64_t g = S->rg[u];
    if (g < 0) return 0;
    const Layout* L = &S->L;
    const Py_ssize_t r = (Py_ssize_t)S->rread[u];
    const int64_t gend = L->goff[r + 1];
    int32_t cb = S->rc[u];
    int moved = 0;
    while (g < gend) {
        const int64_t p = L->plist[g];
        const int64_t e0 = L->off[u] + L->pstart[p];
        const int64_t vb = L->first[S->Q.b[p]];
        const int32_t nb = S->Q.counts[S->Q.b[p]];
        for (; cb < nb; ++cb) {
            const int64_t e = e0 + cb;
            const int live = __atomic_load_n(&S->job.alive[e], __ATOMIC_ACQUIRE);
            if (live && !all && !S->pubd[vb + cb]) {
                S->rg[u] = g;
                S->rc[u] = cb;
                return moved;
            }
            if (live) {
                if (!S->rows[u] && !(S->rows[u] = _PyDict_NewPresized(S->outdeg[u]))) return -1;
                PyObject* d = S->spec[e];
                if (d) {
                    S->spec[e] = NULL;
                    ++S->n_spec_used;
                } else
                    d = attrs_edge(&S->A, S->Q.sc[p], S->Q.en[p]);
                const int bad = !d || PyDict_SetItem(S->rows[u], PyList_GET_ITEM(S->names, vb + cb), d);
                if (bad) {
                    Py_XDECREF(d);
                    return -1;
                }
                /* dptr[e] is read by the head's predecessor cursor, which may still be short of e.  The row holds
                   the dict, so dptr borrows it -- unless some (a, b) pair is listed twice (not a list
                   overlapGraphs.py:43-52 makes, but OverlapEdges accepts it): the second replaces the row's entry
                   and would free the first dict, so then dptr keeps a reference, released at the exit */
                if (!S->own_refs) Py_DECREF(d);
                S->dptr[e] = d;
                ++S->n_ins;
            }
            S->dec[e] = 1;
            ++S->n_dec;
            moved = 1;
            if (pred_advance(S, vb + cb)) return -1;
        }
        ++g;
        cb = 0;
    }
    if (!S->rows[u] && !(S->rows[u] = PyDict_New())) return -1;
    S->rg[u] = -1;
    ++S->n_rows;
    return 1;
}

/* Idle work while the replay runs: the attribute dicts of the still-undecided live out-edges of the nodes from spec_u on,
   made ahead of their rows (row_advance takes them), up to `budget` of them.  Making an edge's dict is about half of
   what inserting it costs, and the edges whose fate the replay decides last -- the graph's last cycles -- are
   otherwise all built after it has ended; an edge removed after its dict was made only costs that dict (released at
   the end).  Each node once, in node order.  Returns the dicts made (0: every node passed), -1 on error. */
static int64_t spec_advance(StreamBuild* S, int64_t budget) {
    const Layout* L = &S->L;
    int64_t made = 0;
    while (S->spec_u < S->N && made < budget) {
        const int64_t u = S->spec_u++;
        int64_t g = S->rg[u];
        if (g < 0 || S->pubd[u]) continue;  /* (row complete, or published: built next) */
        const Py_ssize_t r = (Py_ssize_t)S->rread[u];
        const int64_t gend = L->goff[r + 1];
        int32_t cb = S->rc[u];
        for (; g < gend; ++g, cb = 0) {
            const int64_t p = L->plist[g];
            const int64_t e0 = L->off[u] + L->pstart[p];
            const int32_t nb = S->Q.counts[S->Q.b[p]];
            for (; cb < nb; ++cb) {
                const int64_t e = e0 + cb;
                if (S->spec[e] || !__atomic_load_n(&S->job.alive[e], __ATOMIC_ACQUIRE)) continue;
                PyObject* d = attrs_edge(&S->A, S->Q.sc[p], S->Q.en[p]);
                if (!d) return -1;
                S->spec[e] = d;
                ++made;
            }
        }
    }
    S->n_spec += made;
    return made;
}

/* Idle work once every node has had its dicts made ahead: release the made-ahead dicts of edges the replay has
   removed since, `budget` entries of the edge array per call, cycling over it, so that few are left to release after
   the replay.  Returns the dicts released. */
static int64_t spec_reap(StreamBuild* S, int64_t budget) {
    int64_t freed = 0;
    for (int64_t k = 0; k < budget && S->E > 0; ++k) {
        const int64_t e = S->reap_e++;
        if (S->reap_e >= S->E) S->reap_e = 0;
        PyObject* d = S->spec[e];
        if (d && !__atomic_load_n(&S->job.alive[e], __ATOMIC_ACQUIRE)) {
            S->spec[e] = NULL;
            Py_DECREF(d);
            ++freed;
        }
    }
    return freed;
}

/* The dicts the result is made of, ahead of their contents: every node's successor and predecessor dict not made yet
   (presized to its out- and in-edges, live or not) and the node-ordered top-level dicts (node attributes, succ,
   pred) holding them -- the rows and predecessor dicts are then filled in place.  Idle work while the replay runs
   (otherwise the last step after it), and made before the builder's collections of the young generations, which then
   take these 150 K dicts out of the final one's way.  0, or -1 with an exception set. */
static int make_tops(StreamBuild* S) {
    PyObject* nd = PyDict_New();
    PyObject* sd = PyDict_New();
    PyObject* pd = PyDict_New();
    if (!nd || !sd || !pd) goto fail;
    for (Py_ssize_t i = 0; i < (Py_ssize_t)S->N; ++i) {
        if (!S->rows[i] && !(S->rows[i] = _PyDict_NewPresized(S->outdeg[i]))) goto fail;
        if (!S->pin[i] && !(S->pin[i] = _PyDict_NewPresized(S->pending[i]))) goto fail;
        PyObject* name = PyList_GET_ITEM(S->names, i);
        PyObject* x = PyDict_New();
        const int bad = !x || PyDict_SetItem(nd, name, x) || PyDict_SetItem(sd, name, S->rows[i]) ||
                        PyDict_SetItem(pd, name, S->pin[i]);
        Py_XDECREF(x);
        if (bad) goto fail;
    }
    S->node = nd;
    S->succ = sd;
    S->pred = pd;
    return 0;
fail:
    Py_XDECREF(nd);
    Py_XDECREF(sd);
    Py_XDECREF(pd);
    return -1;
}

/* The collector.  The builder runs with the collector off (millions of new objects), so the first allocation after it
   is back on collects the young generation: every row and predecessor dict built, traversing their millions of
   entries (~0.12 s at the target point on the box, the caller's time).  The builder instead collects the young
   generations itself (gc.collect(1): generations 0 and 1, so the next automatic collection stays a generation-0
   one) in idle time while the replay still runs, when these shares of the edges are decided, leaving only the
   dicts built after the last one for that first collection.  At most kGcMid times: each adds one to generation 2's
   count, whose threshold (10) arms a full collection. */
static const int kGcMid = 3;
static const double kGcAt[3] = {0.30, 0.50, 0.65};

/* the streamed builder's sweeps of its open rows, at most one per this many ms (target point, this container's CPU,
   three runs each: 0 -> 1 ms, build_overlap_stream 1.69-1.79 -> 1.49-1.60 s) */
static const double kSweepMs = 1.0;

static void stream_join(StreamBuild* S) {
    if (S->started) {  /* (it owns no Python objects; the gate: if it still waits for the helper's first pass) */
        __atomic_store_n(&S->job.gate, 1, __ATOMIC_RELEASE);
        pthread_join(S->th, NULL);
        S->started = 0;
    }
    if (S->scc_started) {  /* (it stops once the replay has finished) */
        pthread_join(S->scc_th, NULL);
        S->scc_started = 0;
    }
}

/* The one exit of a streamed build.  Both threads are joined before any buffer they read is released -- on every
   exit, those taken after a thread has started included: an error while the replay runs lets it finish first. */
static void stream_free(StreamBuild* S) {
    if (S->started || S->scc_started) {
        Py_BEGIN_ALLOW_THREADS
        stream_join(S);
        Py_END_ALLOW_THREADS
    }
    PyMem_RawFree(S->scc.nodes);
    PyMem_RawFree(S->job.removed);
    PyMem_RawFree(S->job.alive);
    PyMem_RawFree(S->job.final_nodes);
    if (S->rows)
        for (int64_t i = 0; i < S->N; ++i) Py_XDECREF(S->rows[i]);
    if (S->pin)
        for (int64_t i = 0; i < S->N; ++i) Py_XDECREF(S->pin[i]);
    const double tc0 = S->trace ? now_ms() : 0.0;
    if (S->dptr && S->own_refs)
        for (int64_t e = 0; e < S->E; ++e) Py_XDECREF(S->dptr[e]);
    const double tc1 = S->trace ? now_ms() : 0.0;
    if (S->spec)  /* (the dicts made ahead for edges the replay then removed) */
        for (int64_t e = 0; e < S->E; ++e) Py_XDECREF(S->spec[e]);
    if (S->trace)
        fprintf(stderr, "ovl_stream exit: references %.1f ms, dicts made ahead and unused %.1f ms\n", tc1 - tc0,
                now_ms() - tc1);
    void* const bufs[] = {S->rows, S->pin, S->dptr, S->spec, S->rread, S->bgoff, S->blist, S->pending, S->pg,
                          S->pt,   S->rg,  S->rc,   S->outdeg, S->pubd, S->dec,  S->openl};
    for (size_t i = 0; i < sizeof(bufs) / sizeof(bufs[0]); ++i) PyMem_Free(bufs[i]);
    Py_XDECREF(S->gc_collect);
    Py_XDECREF(S->node);
    Py_XDECREF(S->succ);
    Py_XDECREF(S->pred);
    attrs_free(&S->A);
    layout_free(&S->L);
    pairs_release(&S->Q);
    if (S->off.obj) PyBuffer_Release(&S->off);
    if (S->heads.obj) PyBuffer_Release(&S->heads);
    if (S->w.obj) PyBuffer_Release(&S->w);
}

/* Phase 1: the replay thread on the caller's CSR.  It needs only the CSR, so it starts first and the columns are
   laid out while it runs (the CSR is checked against them there; on a mismatch the replay of the caller's CSR
   still ends, is joined and the call fails). */
static int stream_start_replay(StreamBuild* S, unsigned long long fn_addr) {
    if (S->off.len < 8 || S->heads.len / 4 != S->w.len / 8 || S->off.len / 8 - 1 >= ((Py_ssize_t)1 << 31)) {
        PyErr_SetString(PyExc_ValueError, "names / CSR do not match the columns' graph");
        return -1;
    }
    ReplayJob* j = &S->job;
    S->E = (int64_t)(S->heads.len / 4);
    S->N = (int64_t)(S->off.len / 8 - 1);
    j->fn = (replay_stream_fn)(uintptr_t)fn_addr;
    j->off = (const int64_t*)S->off.buf;
    j->heads = (const int32_t*)S->heads.buf;
    j->w = (const int64_t*)S->w.buf;
    j->n = (int32_t)S->N;
    j->removed = RAW_NEW(int64_t, S->E);
    j->alive = RAW_NEW(uint8_t, S->E);
    j->final_nodes = RAW_NEW(int32_t, S->N);
    if (!j->removed || !j->alive || !j->final_nodes) {
        PyErr_NoMemory();
        return -1;
    }
    /* all ones before either thread starts (the replay sets it too, but on its own thread, where the component
       helper could read it first) */
    memset(j->alive, 1, (size_t)S->E);
    j->cpu_main = sched_getcpu();
    j->gate = S->scc_on != 2;
    if (pthread_create(&S->th, NULL, replay_main, j) != 0) {
        PyErr_SetString(PyExc_RuntimeError, "cannot start the replay thread");
        return -1;
    }
    S->started = 1;
    if (S->trace) S->t_setup = now_ms() - S->t0;
    return 0;
}

/* Phase 2: the columns' layout, checked against the names and the CSR; the in-edge groups; the arrays of dicts;
   the attribute maker and the collector's entry point. */
static int stream_layout(StreamBuild* S, PyObject* shared) {
    const PairCols* Q = &S->Q;
    Layout* L = &S->L;
    if (layout(L, Q)) return -1;
    if (PyList_GET_SIZE(S->names) != L->N || S->N != L->N || S->E != L->E || S->w.len / 8 != L->E ||
        L->N >= ((Py_ssize_t)1 << 31)) {
        PyErr_SetString(PyExc_ValueError, "names / CSR do not match the columns' graph");
        return -1;
    }
    S->rows = NEW0(PyObject*, S->N);
    S->pin = NEW0(PyObject*, S->N);
    S->dptr = NEW0(PyObject*, S->E);
    S->spec = NEW0(PyObject*, S->E);
    S->rread = NEW(int64_t, S->N);
    S->bgoff = NEW0(int64_t, L->R + 1);
    S->blist = NEW(int64_t, L->P);
    S->pending = NEW0(int64_t, S->N);
    int64_t* fill = NEW(int64_t, L->R);
    if (!S->rows || !S->pin || !S->dptr || !S->spec || !S->rread || !S->bgoff || !S->blist || !S->pending || !fill) {
        PyMem_Free(fill);
        PyErr_NoMemory();
        return -1;
    }
    int64_t *bgoff = S->bgoff, *blist = S->blist;
    for (Py_ssize_t r = 0; r < L->R; ++r)
        for (int64_t u = L->first[r]; u < L->first[r + 1]; ++u) S->rread[u] = r;
    for (Py_ssize_t p = 0; p < L->P; ++p)
        if (!Q->keep || Q->keep[p]) ++bgoff[Q->b[p] + 1];
    for (Py_ssize_t r = 0; r < L->R; ++r) bgoff[r + 1] += bgoff[r];
    memcpy(fill, bgoff, sizeof(int64_t) * (size_t)L->R);
    for (Py_ssize_t p = 0; p < L->P; ++p)
        if (!Q->keep || Q->keep[p]) blist[fill[Q->b[p]]++] = p;
    PyMem_Free(fill);
    /* (every copy of one read has the same in-edges) */
    for (Py_ssize_t r = 0; r < L->R; ++r) {
        int64_t k = 0;
        for (int64_t g = bgoff[r]; g < bgoff[r + 1]; ++g) k += L->first[Q->a[blist[g]] + 1] - L->first[Q->a[blist[g]]];
        for (int64_t v = L->first[r]; v < L->first[r + 1]; ++v) S->pending[v] = k;
    }
    if (attrs_init(&S->A, shared)) return -1;
    PyObject* gcm = PyImport_ImportModule("gc");
    if (!gcm) return -1;
    S->gc_collect = PyObject_GetAttrString(gcm, "collect");
    Py_DECREF(gcm);
    if (!S->gc_collect) return -1;
    if (S->trace) S->t_setup = now_ms() - S->t0;  /* (s: the builder's setup done, the replay running since the start) */
    return 0;
}

/* Phase 3: the component helper (scc_main), unless OVL_STREAM_SCC=0 */
static int stream_start_helper(StreamBuild* S) {
    if (!S->scc_on) return 0;
    SccJob* c = &S->scc;
    c->off = S->job.off;
    c->heads = S->job.heads;
    c->alive = S->job.alive;
    c->n = (int32_t)S->N;
    c->stop = &S->job.finished;
    c->gate = &S->job.gate;
    c->nodes = RAW_NEW(int32_t, S->N);
    if (!c->nodes) { PyErr_NoMemory(); return -1; }
    if (pthread_create(&S->scc_th, NULL, scc_main, c) != 0) {
        PyErr_SetString(PyExc_RuntimeError, "cannot start the component thread");
        return -1;
    }
    S->scc_started = 1;
    return 0;
}

/* Phase 4: every node's row and predecessor cursor at its start, and every row open */
static int stream_open_rows(StreamBuild* S) {
    const PairCols* Q = &S->Q;
    const Layout* L = &S->L;
    const int64_t N = S->N;
    S->pg = NEW(int64_t, N);
    S->pt = NEW(int64_t, N);
    S->rg = NEW(int64_t, N);
    S->rc = NEW0(int32_t, N);
    S->outdeg = NEW0(int64_t, N);
    S->pubd = NEW0(uint8_t, N);
    S->dec = NEW0(uint8_t, S->E);
    S->openl = NEW(int64_t, N);
    int32_t* stamp = NEW0(int32_t, L->R);
    if (!S->pg || !S->pt || !S->rg || !S->rc || !S->outdeg || !S->pubd || !S->dec || !S->openl || !stamp) {
        PyMem_Free(stamp);
        PyErr_NoMemory();
        return -1;
    }
    for (int64_t v = 0; v < N; ++v) {
        const Py_ssize_t rv = (Py_ssize_t)S->rread[v];
        const int64_t g0 = S->bgoff[rv];
        S->pg[v] = g0;
        S->pt[v] = g0 < S->bgoff[rv + 1] ? L->first[Q->a[S->blist[g0]]] : 0;
        S->rg[v] = L->goff[rv];
        for (int64_t g = L->goff[rv]; g < L->goff[rv + 1]; ++g) S->outdeg[v] += Q->counts[Q->b[L->plist[g]]];
        S->openl[v] = v;
    }
    /* some read's kept pairs list the same b twice? (then dptr owns its references) */
    int dup = 0;
    for (Py_ssize_t r = 0; r < L->R && !dup; ++r)
        for (int64_t g = L->goff[r]; g < L->goff[r + 1]; ++g) {
            const int32_t bb = Q->b[L->plist[g]];
            if (stamp[bb] == (int32_t)r + 1) { dup = 1; break; }
            stamp[bb] = (int32_t)r + 1;
        }
    PyMem_Free(stamp);
    S->own_refs = dup;
    return 0;
}

/* The publish loop with nothing to build: make attribute dicts ahead; once every node has had its turn, release
   those of removed edges (`reap`) and yield the CPU. */
static int stream_idle(StreamBuild* S, int reap) {
    const int64_t m = spec_advance(S, 256);
    if (m < 0) return -1;
    if (m == 0) {
        if (reap) (void)spec_reap(S, 16384);
        Py_BEGIN_ALLOW_THREADS
        sched_yield();
        Py_END_ALLOW_THREADS
    }
    return 0;
}

/* Phase 5: successors of each node as its out-edges become final (row order: kept pairs with a == its read in
   list order, then the copies of b) -- published by the replay (settled or explored nodes) or by the component
   helper, whichever comes first; predecessors of each node once every tail of its in-edges is.  Ends when the
   replay has finished and every node it published is built. */
static int stream_publish(StreamBuild* S) {
    ReplayJob* job = &S->job;
    SccJob* scc = &S->scc;
    const int64_t N = S->N, E = S->E;
    const int trace = S->trace;
    uint8_t* pubd = S->pubd;
    int64_t *openl = S->openl, *rg = S->rg;
    int64_t k_done = 0, k_scc = 0, n_from_scc = 0, n_sweeps = 0;
    int64_t n_open = N;
    int n_gc = 0;           /* collections of the young generations run so far (kGcMid) */
    double t_sweep = -1e9;  /* the last sweep's start (ms) */
    S->t_replay = S->t_tops = -1.0;
    for (int64_t v = 0; v < N; ++v)
        if (pred_advance(S, v)) return -1;  /* (completes the nodes without in-edges) */
    for (;;) {
        if (trace && S->t_replay < 0.0 && __atomic_load_n(&job->finished, __ATOMIC_ACQUIRE)) {
            S->t_replay = now_ms() - S->t0;
            S->k_at_replay = S->n_rows;
            S->dec_at_replay = S->n_dec;
            S->ins_at_replay = S->n_ins;
        }
        int64_t u = -1;
        if (k_done < __atomic_load_n(&job->n_final, __ATOMIC_ACQUIRE)) {
            u = job->final_nodes[k_done++];
        } else if (S->scc_started && k_scc < __atomic_load_n(&scc->n_pub, __ATOMIC_ACQUIRE)) {
            u = scc->nodes[k_scc++];
            if (!pubd[u]) ++n_from_scc;
        }
        if (u >= 0) {
            if (pubd[u]) continue;  /* (published by both) */
            pubd[u] = 1;
            if (row_advance(S, u, 1) < 0) return -1;
            continue;
        }
        if (__atomic_load_n(&job->finished, __ATOMIC_ACQUIRE)) {
            if (__atomic_load_n(&job->n_final, __ATOMIC_ACQUIRE) > k_done) continue;
            break;
        }
        /* nothing newly published: advance the open rows as far as their heads allow -- at most once per
           kSweepMs (a sweep calls row_advance on every open row, hundreds of millions of calls over a run when
           repeated back to back); in between, and after a sweep that moved nothing, make attribute dicts ahead */
        if (now_ms() - t_sweep < kSweepMs) {
            if (!S->node) {  /* first: every row and predecessor dict and the top-level dicts, once */
                if (make_tops(S)) return -1;
                if (trace) S->t_tops = now_ms() - S->t0;
                continue;
            }
            if (n_gc < kGcMid && S->n_dec >= (int64_t)(kGcAt[n_gc] * (double)E)) {
                /* the collector's pass over the dicts built so far, now, beside the replay (see kGcMid) */
                const double tg = now_ms();
                PyObject* res = PyObject_CallFunction(S->gc_collect, "i", 1);
                if (!res) return -1;
                Py_DECREF(res);
                S->t_gc += now_ms() - tg;
                ++n_gc;
                continue;
            }
            if (stream_idle(S, 1)) return -1;
            continue;
        }
        t_sweep = now_ms();
        int moved = 0;
        int64_t keep_n = 0;
        for (int64_t i = 0; i < n_open; ++i) {
            const int64_t x = openl[i];
            if (rg[x] < 0) continue;
            const int m = row_advance(S, x, 0);
            if (m < 0) return -1;
            moved |= m;
            if (rg[x] >= 0) openl[keep_n++] = x;
            if ((i & 255) == 255 && k_done < __atomic_load_n(&job->n_final, __ATOMIC_ACQUIRE)) {
                /* (newly published nodes first: keep the rest of the list for the next sweep) */
                for (int64_t j = i + 1; j < n_open; ++j) openl[keep_n++] = openl[j];
                break;
            }
        }
        n_open = keep_n;
        ++n_sweeps;
        if (!moved && stream_idle(S, 0)) return -1;  /* (nothing to insert yet) */
    }
    S->k_done = k_done;
    S->n_from_scc = n_from_scc;
    S->n_sweeps = n_sweeps;
    S->n_gc = n_gc;
    return 0;
}

/* Phase 6: both threads joined, the replay's verdict, the top-level dicts if idle time did not make them, the
   trace line and the result tuple (NULL with an exception set on failure) */
static PyObject* stream_finish(StreamBuild* S) {
    const ReplayJob* job = &S->job;
    const int64_t N = S->N, E = S->E;
    stream_join(S);
    if (S->trace) S->t_built = now_ms() - S->t0;
    if (job->rc != 0 || S->k_done != N || S->n_rows != N || S->n_pred != N) {
        PyErr_Format(PyExc_RuntimeError, "ovl_remove_cycles_stream failed (rc %d, %lld of %lld nodes final, "
                     "%lld predecessor dicts)", job->rc, (long long)S->k_done, (long long)N, (long long)S->n_pred);
        return NULL;
    }
    if (!S->node && make_tops(S)) return NULL;
    PyObject* rem = PyBytes_FromStringAndSize((const char*)job->removed, (Py_ssize_t)(8 * job->n_removed));
    if (!rem) return NULL;
    PyObject* out = Py_BuildValue("(OOONL)", S->node, S->succ, S->pred, rem, (long long)job->n_removed);
    if (S->trace) {
        const double dec_pct = E ? 100.0 * (double)S->dec_at_replay / (double)E : 0.0;
        fprintf(stderr,
                "ovl_stream: s=%.1f r=%.1f (%.0f%% rows, %.0f%% edges, %lld inserted) b=%.1f t=%.1f sweeps=%lld "
                "scc=%d passes=%d first=%lld replay=%.1f cpus main %d/%d replay %d/%d spec %lld used %lld "
                "gc %d in %.1f ms tops at %.1f dec %.0f%%\n",
                S->t_setup, S->t_replay, N ? 100.0 * (double)S->k_at_replay / (double)N : 100.0,
                E ? dec_pct : 100.0, (long long)S->ins_at_replay, S->t_built, now_ms() - S->t0,
                (long long)S->n_sweeps, S->scc_on, S->scc.passes, (long long)S->n_from_scc, job->ms, job->cpu_main,
                sched_getcpu(), job->cpu_start, job->cpu_end, (long long)S->n_spec, (long long)S->n_spec_used,
                S->n_gc, S->t_gc, S->t_tops, dec_pct);
    }
    return out;
}

static PyObject* build_overlap_stream_impl(PyObject* self, PyObject* args) {
    (void)self;
    PyObject *names, *oc, *oa, *ob, *os, *oe, *ok, *shared, *ooff, *oh, *ow;
    unsigned long long fn_addr;
    if (!PyArg_ParseTuple(args, "O!OOOOOOOKOOO", &PyList_Type, &names, &oc, &oa, &ob, &os, &oe, &ok, &shared,
                          &fn_addr, &ooff, &oh, &ow))
        return NULL;
    StreamBuild S;
    memset(&S, 0, sizeof(S));
    S.names = names;
    S.own_refs = 1;
    const char* scc_env = getenv("OVL_STREAM_SCC");
    S.scc_on = scc_env ? atoi(scc_env) : 1;
    const char* tr_env = getenv("OVL_TRACE_STREAM");
    S.trace = tr_env && atoi(tr_env) != 0;
    S.t0 = S.trace ? now_ms() : 0.0;
    PyObject* out = NULL;
    if (pairs_take(&S.Q, oc, oa, ob, os, oe, ok) == 0 && take(ooff, &S.off, 8, "off") == 0 &&
        take(oh, &S.heads, 4, "heads") == 0 && take(ow, &S.w, 8, "weights") == 0 &&
        stream_start_replay(&S, fn_addr) == 0 &&  /* first: the layout runs beside it */
        stream_layout(&S, shared) == 0 &&
        stream_start_helper(&S) == 0 &&
        stream_open_rows(&S) == 0 &&
        stream_publish(&S) == 0)
        out = stream_finish(&S);
    stream_free(&S);
    return out;
}

// ----------------------------------------------------------------------------- pooled object arenas
//
// The graph's dicts (an attribute dict per edge, a row and a predecessor dict per node: ~2.3 M objects at the
// target point, ~0.4 GB) come from CPython's object arenas (256 KiB each, one mmap per arena).  Fresh arenas land on
// pages the kernel must fault in and zero, 4 KiB at a time: ~2·10^5 minor faults in a process's first removal.
// While a builder call runs (build, build_overlap, build_overlap_stream: pool_scope), an arena allocator carves
// arenas from 64 MiB regions aligned to 2 MiB and advised for transparent huge pages (far fewer faults), and arenas
// freed meanwhile go on a free list for the call's own later dicts.  The previous allocator is restored when the
// call returns, so the pool touches nothing else in the process: the graph's arenas go back to the kernel by
// CPython's own munmap when the graph is freed, and of the free list at most kPoolKeep arenas stay mapped for the
// next call (the rest are unmapped).  OVL_ARENA_POOL=0: builder calls keep CPython's allocator.
#include <sys/mman.h>

#define OVL_POOL_REGION (64u << 20)
#define OVL_POOL_MAX_REGIONS 1024
#define OVL_POOL_KEEP 256  // freed arenas kept mapped across builder calls (64 MiB of 256 KiB arenas)

static PyObjectArenaAllocator g_prev_arena;
static int g_pool_enabled = -1;   // OVL_ARENA_POOL (read once): 0 off, else on
static int g_pool_depth = 0;      // builder calls in progress (the allocator is installed while > 0)
static void* g_pool_free = NULL;  // freed pool arenas, linked through their first word
static size_t g_pool_nfree = 0;
static char* g_pool_cur = NULL;
static size_t g_pool_left = 0;
static size_t g_pool_arena = 0;  // the arena size CPython asks for (the first request's)
static char* g_region_base[OVL_POOL_MAX_REGIONS];  // ascending
static int g_regions = 0;
static size_t g_pool_mapped = 0, g_pool_reused = 0, g_pool_released = 0;

static int pool_owns(const void* p) {  // (binary search over the ascending region bases)
    int lo = 0, hi = g_regions;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if ((const char*)p < g_region_base[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo > 0 && (const char*)p < g_region_base[lo - 1] + OVL_POOL_REGION;
}

static void* pool_arena_alloc(void* ctx, size_t size) {
    (void)ctx;
    if (!g_pool_arena) g_pool_arena = size;
    if (size != g_pool_arena || size > OVL_POOL_REGION) return g_prev_arena.alloc(g_prev_arena.ctx, size);
    if (g_pool_free) {
        void* p = g_pool_free;
        g_pool_free = *(void**)p;
        --g_pool_nfree;
        ++g_pool_reused;
        return p;
    }
    if (g_pool_left < size) {
        if (g_regions == OVL_POOL_MAX_REGIONS) return g_prev_arena.alloc(g_prev_arena.ctx, size);
        const size_t huge = (size_t)2 << 20;
        char* m = (char*)mmap(NULL, OVL_POOL_REGION + huge, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == (char*)MAP_FAILED) return g_prev_arena.alloc(g_prev_arena.ctx, size);
        char* a = (char*)(((uintptr_t)m + huge - 1) & ~(uintptr_t)(huge - 1));
        if (a > m) munmap(m, (size_t)(a - m));                               // trim to the aligned region
        if (a + OVL_POOL_REGION < m + OVL_POOL_REGION + huge)
            munmap(a + OVL_POOL_REGION, (size_t)(m + OVL_POOL_REGION + huge - (a + OVL_POOL_REGION)));
#ifdef MADV_HUGEPAGE
        madvise(a, OVL_POOL_REGION, MADV_HUGEPAGE);
#endif
        int i = g_regions++;
        for (; i > 0 && g_region_base[i - 1] > a; --i) g_region_base[i] = g_region_base[i - 1];
        g_region_base[i] = a;
        g_pool_cur = a;
        g_pool_left = OVL_POOL_REGION;
        g_pool_mapped += OVL_POOL_REGION;
    }
    void* p = g_pool_cur;
    g_pool_cur += size;
    g_pool_left -= size;
    return p;
}

static void pool_arena_free(void* ctx, void* p, size_t size) {
    (void)ctx;
    if (p && size == g_pool_arena && pool_owns(p)) {
        *(void**)p = g_pool_free;
        g_pool_free = p;
        ++g_pool_nfree;
        return;
    }
    g_prev_arena.free(g_prev_arena.ctx, p, size);
}

// a builder call's start / end (with the GIL held): install the pool / trim its free list and restore CPython's
static void pool_begin(void) {
    if (g_pool_enabled < 0) {
        const char* e = getenv("OVL_ARENA_POOL");
        g_pool_enabled = !(e && !strcmp(e, "0"));
    }
    if (!g_pool_enabled || g_pool_depth++ > 0) return;
    PyObjectArenaAllocator mine = {NULL, pool_arena_alloc, pool_arena_free};
    PyObject_GetArenaAllocator(&g_prev_arena);
    PyObject_SetArenaAllocator(&mine);
}

static void pool_end(void) {
    if (!g_pool_enabled || g_pool_depth == 0 || --g_pool_depth > 0) return;
    void* keep = NULL;
    void** tail = &keep;
    size_t kept = 0;
    for (void* p = g_pool_free; p;) {
        void* next = *(void**)p;
        if (kept < OVL_POOL_KEEP) {
            *tail = p;
            tail = (void**)p;
            ++kept;
        } else {
            munmap(p, g_pool_arena);  // (its addresses are never handed out again: off the list, below g_pool_cur)
            ++g_pool_released;
        }
        p = next;
    }
    *tail = NULL;
    g_pool_free = keep;
    g_pool_nfree = kept;
    PyObject_SetArenaAllocator(&g_prev_arena);
}

// stats (tests): {on: installed now, enabled, arena_bytes, mapped_bytes, reused_arenas, kept_arenas, released_arenas}
static PyObject* arena_pool(PyObject* self, PyObject* args) {
    (void)self;
    (void)args;
    return Py_BuildValue("{s:i,s:i,s:n,s:n,s:n,s:n,s:n}", "on", g_pool_depth > 0 ? 1 : 0, "enabled", g_pool_enabled,
                         "arena_bytes", (Py_ssize_t)g_pool_arena, "mapped_bytes", (Py_ssize_t)g_pool_mapped,
                         "reused_arenas", (Py_ssize_t)g_pool_reused, "kept_arenas", (Py_ssize_t)g_pool_nfree,
                         "released_arenas", (Py_ssize_t)g_pool_released);
}

// the builder entry points, each inside a pool scope
#define OVL_POOL_SCOPED(name)                                  \
    static PyObject* name(PyObject* self, PyObject* args) {    \
        pool_begin();                                          \
        PyObject* r = name##_impl(self, args);                 \
        pool_end();                                            \
        return r;                                              \
    }
OVL_POOL_SCOPED(build)
OVL_POOL_SCOPED(build_overlap)
OVL_POOL_SCOPED(build_overlap_stream)

static PyMethodDef methods[] = {
    {"arena_pool", arena_pool, METH_VARARGS,
     "arena_pool() -> stats of the pooled, huge-page-advised object arenas builder calls allocate from"},
    {"overlap_csr", overlap_csr, METH_VARARGS,
     "overlap_csr(counts, a, b, score[, keep]) -> (off int64, heads int32, weights int64) bytearrays"},
    {"build_overlap_stream", build_overlap_stream, METH_VARARGS,
     "build_overlap_stream(names, counts, a, b, score, end, keep, shared, replay_fn, off, heads, weights) -> "
     "(node, succ, pred, removed, n_removed)"},
    {"build_overlap", build_overlap, METH_VARARGS,
     "build_overlap(names, counts, a, b, score, end[, keep[, alive[, shared]]]) -> (node, succ, pred)"},
    {"build", build, METH_VARARGS, "build(names, u, v, weight, end) -> (node, succ, pred) dicts of a networkx DiGraph"},
    {"csr", csr, METH_VARARGS, "csr(nodes, adj[, more int types]) -> (off int64, heads int32, weights int64) bytearrays"},
    {"remove_edges", remove_edges, METH_VARARGS, "remove_edges(succ, pred, nodes, tails, heads): bulk remove_edge"},
    {NULL, NULL, 0, NULL},
};

static struct PyModuleDef module = {PyModuleDef_HEAD_INIT, "_digraph", NULL, -1, methods, NULL, NULL, NULL, NULL};

PyMODINIT_FUNC PyInit__digraph(void) { return PyModule_Create(&module); }
