// _internal.cpp -- CPython extension `gf2bv_amd._internal`.
//
// Mirrors the native boundary of the reference (maple3142/gf2bv, gf2bv/_internal.c:767-833):
// same callables (m4ri_solve, to_bits, xor_tuple, tuple_where, mul_bit_quad), same types
// (AffineSpace, AffineSpaceIterator, AffineSpaceIteratorSlow), same argument meaning and
// error behaviour -- but m4ri_solve hands the equations to libgf2bv_hip.so (HIP kernels on
// MI355X) instead of M4RI.  No GF(2) elimination happens in this file and there is no CPU
// fallback: without a GPU m4ri_solve raises RuntimeError.
//
// Host-side work kept here, as in the reference: reading CPython int digits
// (_internal.c:5-16, 41-59 -- here a memcpy of ob_digit, the bit shuffling is the device pack
// kernel), converting word vectors back to ints (_internal.c:32-39) and the tiny
// origin ^ basis[i] combinations of AffineSpace.get / iteration (_internal.c:101-122, 242-273).
#define PY_SSIZE_T_CLEAN
#include <Python.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/gf2bv_hip.h"

#if PY_VERSION_HEX >= 0x030C0000
#define GF2_DIGIT_COUNT(o) ((Py_ssize_t)((o)->long_value.lv_tag >> 3))
#define GF2_DIGITS(o) ((o)->long_value.ob_digit)
#else
#define GF2_DIGIT_COUNT(o) (Py_SIZE(o) < 0 ? -Py_SIZE(o) : Py_SIZE(o))
#define GF2_DIGITS(o) ((o)->ob_digit)
#endif

namespace {

PyObject *words_to_pylong(const uint64_t *w, int64_t nwords)
{
	if (nwords <= 0) return PyLong_FromLong(0);
	return _PyLong_FromByteArray(reinterpret_cast<const unsigned char *>(w), (size_t)nwords * 8, 1, 0);
}

// bit `i` (LSB = 0) of |v|, false beyond its digits
inline bool long_bit(PyLongObject *v, Py_ssize_t i)
{
	Py_ssize_t d = i / PyLong_SHIFT;
	if (d >= GF2_DIGIT_COUNT(v)) return false;
	return (GF2_DIGITS(v)[d] >> (i % PyLong_SHIFT)) & 1;
}

// ------------------------------------------------------------------------------------------------
// AffineSpace: origin + basis as 64-bit word vectors (the reference keeps two mzd_t*,
// gf2bv/_internal.h:7-10).
struct AffineSpaceObject {
	PyObject_HEAD
	int64_t dim, words;
	uint64_t *origin;   // words
	uint64_t *basis;    // dim x words
	int device;         // the device whose solve produced the space (its large walks are materialised there);
	                    // -1: built from host integers by the test hook _space_from_ints -- walked on the host
};

struct SpaceIterObject {
	PyObject_HEAD
	AffineSpaceObject *space;
	uint64_t *cur;      // Gray: running vector; Slow: scratch
	uint64_t idx;       // Gray index
	uint8_t *state;     // Slow: dim+1 counter bits
	int done;
	// Large spaces: the elements are materialised on the device a chunk at a time (gf2bv_space_enumerate) and the
	// iterator only slices ints out of the chunk -- no per-item XOR on the host.  Small ones (a chunk would be under
	// 64 KiB) are stepped on the host as in the reference: a kernel launch costs more than their whole walk.
	gf2bv_space *dev;   // nullptr: host stepping
	const uint64_t *chunk;   // the space handle's pinned buffer, filled by the last gf2bv_space_enumerate
	int64_t chunk_cap, chunk_fill, chunk_pos;
	uint64_t next_first;     // index of the first element of the next chunk
	int wrapped;             // next_first has run past 2^64 - 1 (dimension 64 only)
};

constexpr int64_t kChunkBytes = 8 << 20, kDeviceMinBytes = 64 << 10;

PyTypeObject *AffineSpace_Type, *SpaceIterGray_Type, *SpaceIterSlow_Type;

void space_dealloc(AffineSpaceObject *self)
{
	PyTypeObject *tp = Py_TYPE(self);
	free(self->origin);
	free(self->basis);
	tp->tp_free((PyObject *)self);
	Py_DECREF(tp);
}

PyObject *space_dimension(AffineSpaceObject *self, void *) { return PyLong_FromLongLong(self->dim); }
PyObject *space_device(AffineSpaceObject *self, void *) { return PyLong_FromLong(self->device); }
PyObject *space_origin(AffineSpaceObject *self, void *) { return words_to_pylong(self->origin, self->words); }
PyObject *space_basis(AffineSpaceObject *self, void *)
{
	PyObject *t = PyTuple_New(self->dim);   // a tuple, like _internal.c:218-230 (the .pyi says list)
	if (!t) return nullptr;
	for (int64_t i = 0; i < self->dim; i++) {
		PyObject *v = words_to_pylong(self->basis + i * self->words, self->words);
		if (!v) { Py_DECREF(t); return nullptr; }
		PyTuple_SET_ITEM(t, i, v);
	}
	return t;
}

// AffineSpace.get(n): origin ^ XOR of basis rows at the set bits of n (binary, not Gray; only
// the low `dimension` bits of |n| are read) -- _internal.c:242-273
PyObject *space_get(AffineSpaceObject *self, PyObject *const *args, Py_ssize_t nargs)
{
	if (nargs != 1) { PyErr_SetString(PyExc_TypeError, "get requires 1 argument"); return nullptr; }
	if (!PyLong_Check(args[0])) { PyErr_SetString(PyExc_TypeError, "Index must be an integer"); return nullptr; }
	PyLongObject *n = (PyLongObject *)args[0];
	int64_t sw = (self->dim + 63) / 64;
	std::vector<uint64_t> sel((size_t)(sw ? sw : 1), 0), out((size_t)(self->words ? self->words : 1), 0);
	for (int64_t i = 0; i < self->dim; i++)
		if (long_bit(n, i)) sel[i >> 6] |= (uint64_t)1 << (i & 63);
	gf2bv_space_combine(self->origin, self->basis, self->dim, self->words, sel.data(), sw, out.data());
	return words_to_pylong(out.data(), self->words);
}

PyObject *space_iter(AffineSpaceObject *self)
{
	const bool gray = self->dim <= 64;       // _internal.c:185
	PyTypeObject *tp = gray ? SpaceIterGray_Type : SpaceIterSlow_Type;
	SpaceIterObject *it = (SpaceIterObject *)tp->tp_alloc(tp, 0);
	if (!it) return nullptr;
	Py_INCREF(self);
	it->space = self;
	it->idx = 0;
	it->done = 0;
	it->state = nullptr;
	size_t nw = (size_t)(self->words ? self->words : 1);
	it->dev = nullptr; it->chunk = nullptr; it->chunk_cap = it->chunk_fill = it->chunk_pos = 0; it->next_first = 0; it->wrapped = 0;
	it->cur = (uint64_t *)malloc(nw * sizeof(uint64_t));
	if (!gray) it->state = (uint8_t *)calloc((size_t)self->dim + 1, 1);
	if (!it->cur || (!gray && !it->state)) { Py_DECREF(it); return PyErr_NoMemory(); }
	memcpy(it->cur, self->origin, (size_t)self->words * sizeof(uint64_t));
	// device enumeration when a chunk is worth a launch: min(2^dim, chunk capacity) elements of `words` words
	const int64_t row_bytes = (int64_t)nw * 8;
	int64_t cap = std::max<int64_t>(1, kChunkBytes / row_bytes);
	if (self->dim < 40) cap = std::min<int64_t>(cap, (int64_t)1 << self->dim);
	if (self->device >= 0 && self->words > 0 && cap * row_bytes >= kDeviceMinBytes) {
		if (gf2bv_space_open(self->origin, self->basis, self->dim, self->words, self->device, &it->dev) != GF2BV_OK) {
			PyErr_SetString(PyExc_RuntimeError, gf2bv_last_error());
			Py_DECREF(it);
			return nullptr;
		}
		it->chunk_cap = cap;
	}
	return (PyObject *)it;
}

// total number of elements still to be produced from index `first` on, capped at `cap` (2^dim may not fit 64 bits)
int64_t remaining_from(int64_t dim, uint64_t first, int wrapped, int64_t cap)
{
	if (wrapped) return 0;
	if (dim >= 64) {                                   // 2^64 (or more) elements: only the wrap ends the walk
		const uint64_t left = ~first;                  // elements first .. 2^64 - 1 = left + 1
		return (left >= (uint64_t)cap) ? cap : (int64_t)left + 1;
	}
	const uint64_t total = (uint64_t)1 << dim;
	if (first >= total) return 0;
	return (int64_t)std::min<uint64_t>(total - first, (uint64_t)cap);
}

// next element from the device-filled chunk; refills when it runs dry.  Returns nullptr with no error set at the end.
PyObject *iter_next_chunked(SpaceIterObject *self, int gray)
{
	AffineSpaceObject *sp = self->space;
	if (self->chunk_pos >= self->chunk_fill) {
		// (binary walk with dimension > 64: the first 2^64 elements only involve basis[0..63]; nobody gets further)
		const int64_t n = remaining_from(sp->dim, self->next_first, self->wrapped, self->chunk_cap);
		if (n <= 0) return nullptr;
		int rc;
		Py_BEGIN_ALLOW_THREADS
		rc = gf2bv_space_enumerate(self->dev, self->next_first, n, gray, nullptr);
		Py_END_ALLOW_THREADS
		if (rc != GF2BV_OK) { PyErr_SetString(PyExc_RuntimeError, gf2bv_last_error()); return nullptr; }
		self->chunk = gf2bv_space_buffer(self->dev);
		const uint64_t before = self->next_first;
		self->next_first += (uint64_t)n;
		if (self->next_first < before || (sp->dim >= 64 && self->next_first == 0)) self->wrapped = 1;
		self->chunk_fill = n; self->chunk_pos = 0;
	}
	return words_to_pylong(self->chunk + self->chunk_pos++ * sp->words, sp->words);
}

void iter_dealloc(SpaceIterObject *self)
{
	PyTypeObject *tp = Py_TYPE(self);
	Py_XDECREF(self->space);
	if (self->dev) gf2bv_space_close(self->dev);
	free(self->cur);
	free(self->state);
	tp->tp_free((PyObject *)self);
	Py_DECREF(tp);
}

// Reflected Gray code walk, _internal.c:101-122: yield the running vector, then flip the basis
// row whose index is the bit in which gray(idx) and gray(idx+1) differ.
PyObject *iter_next_gray(SpaceIterObject *self)
{
	if (self->dev) return iter_next_chunked(self, 1);
	if (self->done) return nullptr;
	AffineSpaceObject *sp = self->space;
	PyObject *ret = words_to_pylong(self->cur, sp->words);
	uint64_t x = self->idx ^ (self->idx >> 1);
	self->idx++;
	uint64_t y = self->idx ^ (self->idx >> 1);
	int diff = __builtin_ctzll(x ^ y);
	if (diff >= sp->dim || (sp->dim == 64 && self->idx == 0)) {
		self->done = 1;
		return ret;
	}
	const uint64_t *b = sp->basis + (int64_t)diff * sp->words;
	for (int64_t w = 0; w < sp->words; w++) self->cur[w] ^= b[w];
	return ret;
}

// Binary counter walk for dimension > 64, _internal.c:63-91 (basis[0] is the LSB).
PyObject *iter_next_slow(SpaceIterObject *self)
{
	if (self->dev) return iter_next_chunked(self, 0);
	AffineSpaceObject *sp = self->space;
	const int64_t n = sp->dim;
	if (self->state[n]) return nullptr;
	memcpy(self->cur, sp->origin, (size_t)sp->words * sizeof(uint64_t));
	for (int64_t r = 0; r < n; r++)
		if (self->state[r])
			for (int64_t w = 0; w < sp->words; w++) self->cur[w] ^= sp->basis[r * sp->words + w];
	uint8_t sentinel = 1;
	for (int64_t r = 0; r < n; r++) {
		self->state[r] ^= 1;
		if (self->state[r]) { sentinel = 0; break; }
	}
	self->state[n] = sentinel;
	return words_to_pylong(self->cur, sp->words);
}

PyObject *QuadGaveUp;      // _internal.QuadSearchGaveUp(message, lin_rank)
PyObject *CubicGaveUp;     // _internal.CubicSearchGaveUp(message, lin_rank)
PyObject *QuarticGaveUp;   // _internal.QuarticSearchGaveUp(message, lin_rank)
PyObject *space_quad_search(AffineSpaceObject *self, PyObject *const *args, Py_ssize_t nargs);
PyObject *space_cubic_search(AffineSpaceObject *self, PyObject *const *args, Py_ssize_t nargs);
PyObject *space_quartic_search(AffineSpaceObject *self, PyObject *const *args, Py_ssize_t nargs);

PyGetSetDef space_getset[] = {
	{"dimension", (getter)space_dimension, nullptr, "Dimension of the affine space", nullptr},
	{"origin", (getter)space_origin, nullptr, "Origin of the affine space", nullptr},
	{"basis", (getter)space_basis, nullptr, "Basis of the affine space", nullptr},
	{"device", (getter)space_device, nullptr, "GPU whose solve produced the space (-1: built on the host); not in the reference", nullptr},
	{nullptr, nullptr, nullptr, nullptr, nullptr}};

PyMethodDef space_methods[] = {
	{"get", (PyCFunction)(void (*)(void))space_get, METH_FASTCALL,
	 "get(n)\n--\n\nGet the n-th element of the affine space, should check 0 <= n < 2**(space.dimension) first."},
	{"quad_search", (PyCFunction)(void (*)(void))space_quad_search, METH_FASTCALL,
	 "quad_search(n_lin, max_enum=32, max_solutions=65536, first=False)\n--\n\nThe consistent points of a QuadraticSystem space (product "
	 "coordinates = products of the n_lin linear bits), in iteration order, searched on the GPU (first=True: the first max_solutions of "
	 "them, however many there are); not in the reference."},
	{"cubic_search", (PyCFunction)(void (*)(void))space_cubic_search, METH_FASTCALL,
	 "cubic_search(n_lin, max_enum=32, max_solutions=65536, first=False)\n--\n\nquad_search for a space over the degree-3 columns (pair "
	 "and triple coordinates = products of the n_lin linear bits): degree-3 XL's and PackedCubicSystem's; not in the reference."},
	{"quartic_search", (PyCFunction)(void (*)(void))space_quartic_search, METH_FASTCALL,
	 "quartic_search(n_lin, max_enum=32, max_solutions=65536, first=False)\n--\n\nquad_search for a space over the degree-4 columns (pair, "
	 "triple and quadruple coordinates = products of the n_lin linear bits): degree-4 XL's and PackedQuarticSystem's; not in the reference."},
	{nullptr, nullptr, 0, nullptr}};

PyType_Slot space_slots[] = {
	{Py_tp_dealloc, (void *)space_dealloc}, {Py_tp_iter, (void *)space_iter},
	{Py_tp_methods, (void *)space_methods}, {Py_tp_getset, (void *)space_getset}, {0, nullptr}};
PyType_Slot gray_slots[] = {
	{Py_tp_dealloc, (void *)iter_dealloc}, {Py_tp_iter, (void *)PyObject_SelfIter},
	{Py_tp_iternext, (void *)iter_next_gray}, {0, nullptr}};
PyType_Slot slow_slots[] = {
	{Py_tp_dealloc, (void *)iter_dealloc}, {Py_tp_iter, (void *)PyObject_SelfIter},
	{Py_tp_iternext, (void *)iter_next_slow}, {0, nullptr}};

#ifndef Py_TPFLAGS_DISALLOW_INSTANTIATION
#define Py_TPFLAGS_DISALLOW_INSTANTIATION 0
#endif
PyType_Spec space_spec = {"_internal.AffineSpace", sizeof(AffineSpaceObject), 0,
                          Py_TPFLAGS_DEFAULT | Py_TPFLAGS_DISALLOW_INSTANTIATION, space_slots};
PyType_Spec gray_spec = {"_internal.AffineSpaceIterator", sizeof(SpaceIterObject), 0,
                         Py_TPFLAGS_DEFAULT | Py_TPFLAGS_DISALLOW_INSTANTIATION, gray_slots};
PyType_Spec slow_spec = {"_internal.AffineSpaceIteratorSlow", sizeof(SpaceIterObject), 0,
                         Py_TPFLAGS_DEFAULT | Py_TPFLAGS_DISALLOW_INSTANTIATION, slow_slots};

// Result handle -> None / int / AffineSpace (_internal.c:440-501); frees the handle.
PyObject *result_to_py(gf2bv_result *res, long mode, int device)
{
	if (gf2bv_result_status(res) != GF2BV_STATUS_SOLVED) {
		gf2bv_result_free(res);
		Py_RETURN_NONE;              // inconsistent system -> None (_internal.c:440-446)
	}
	const int64_t words = gf2bv_result_words(res);
	PyObject *ret = nullptr;
	if (mode == GF2BV_MODE_SINGLE) {
		std::vector<uint64_t> o((size_t)(words ? words : 1));
		gf2bv_result_origin(res, o.data());
		ret = words_to_pylong(o.data(), words);
	} else {
		AffineSpaceObject *sp = (AffineSpaceObject *)AffineSpace_Type->tp_alloc(AffineSpace_Type, 0);
		if (sp) {
			sp->dim = gf2bv_result_dimension(res);
			sp->words = words;
			sp->device = device;
			sp->origin = (uint64_t *)calloc((size_t)(words ? words : 1), sizeof(uint64_t));
			sp->basis = (uint64_t *)calloc((size_t)((sp->dim * words) > 0 ? sp->dim * words : 1), sizeof(uint64_t));
			if (!sp->origin || !sp->basis) {
				Py_DECREF(sp);                   // (space_dealloc frees whichever half exists)
				gf2bv_result_free(res);
				return PyErr_NoMemory();
			}
			gf2bv_result_origin(res, sp->origin);
			gf2bv_result_basis(res, sp->basis);
			ret = (PyObject *)sp;
		}
	}
	gf2bv_result_free(res);
	return ret;
}

// Which GPU a solve runs on.  The reference's m4ri_solve has no such notion (one core of the host); here every solve entry
// takes an OPTIONAL trailing `device` argument (an index below device_count()), and without it uses the module default
// (set_default_device; initially the environment variable GF2BV_DEVICE, else 0).  AffineSpace remembers the device of
// its solve: large walks are materialised there.
int g_default_device = -1;
int default_device()
{
	if (g_default_device < 0) {
		const char *e = getenv("GF2BV_DEVICE");
		g_default_device = e ? atoi(e) : 0;
		if (g_default_device < 0) g_default_device = 0;
	}
	return g_default_device;
}
bool parse_device(PyObject *obj, int *device)
{
	if (obj == Py_None) { *device = default_device(); return true; }
	const long d = PyLong_AsLong(obj);
	if (d == -1 && PyErr_Occurred()) return false;
	const int n = gf2bv_device_count();
	if (d < 0 || (n > 0 && d >= n)) { PyErr_Format(PyExc_ValueError, "device %ld out of range (%d visible)", d, n); return false; }
	*device = (int)d;
	return true;
}
// devices: None = the module's default device (set_default_device / GF2BV_DEVICE -- what m4ri_solve and m4ri_solve_packed use:
// a process pinned to one GPU stays on it), the string "all" = every visible device, an int, or a sequence of ints (repeats allowed)
bool parse_devices(PyObject *obj, std::vector<int> *devs)
{
	devs->clear();
	if (obj == Py_None) { devs->push_back(default_device()); return true; }
	if (PyUnicode_Check(obj)) {
		if (PyUnicode_CompareWithASCIIString(obj, "all") != 0) {
			PyErr_SetString(PyExc_ValueError, "devices must be None, 'all', an int or a sequence of ints");
			return false;
		}
		const int n = gf2bv_device_count();
		for (int d = 0; d < (n > 0 ? n : 1); d++) devs->push_back(d);
		return true;
	}
	if (PyLong_Check(obj)) { int d; if (!parse_device(obj, &d)) return false; devs->push_back(d); return true; }
	PyObject *seq = PySequence_Fast(obj, "devices must be None, 'all', an int or a sequence of ints");
	if (!seq) return false;
	const Py_ssize_t n = PySequence_Fast_GET_SIZE(seq);
	for (Py_ssize_t i = 0; i < n; i++) {
		int d;
		if (!parse_device(PySequence_Fast_GET_ITEM(seq, i), &d)) { Py_DECREF(seq); return false; }
		devs->push_back(d);
	}
	Py_DECREF(seq);
	if (devs->empty()) { PyErr_SetString(PyExc_ValueError, "devices must not be empty"); return false; }
	return true;
}

// cols / mode checks of every solve entry (_internal.c:372-395)
bool parse_mode(PyObject *obj, long *mode)
{
	*mode = PyLong_AsLong(obj);
	if (*mode == -1 && PyErr_Occurred()) return false;
	if (*mode != GF2BV_MODE_SINGLE && *mode != GF2BV_MODE_AFFINE_SPACE) { PyErr_SetString(PyExc_ValueError, "Invalid mode"); return false; }
	return true;
}
bool parse_cols_mode(PyObject *cols_obj, PyObject *mode_obj, Py_ssize_t *cols, long *mode)
{
	*cols = PyLong_AsSsize_t(cols_obj);
	if (*cols <= 0) {
		if (*cols == -1 && PyErr_Occurred()) return false;
		PyErr_SetString(PyExc_ValueError, "Number of columns must be positive");
		return false;
	}
	return parse_mode(mode_obj, mode);
}

// ... and the rows they need (after parse_cols_mode)
bool rows_cover_cols(Py_ssize_t rows, Py_ssize_t cols)
{
	if (rows >= cols) return true;
	PyErr_SetString(PyExc_ValueError, "Number of rows must be greater than or equal to number of columns, try pad with zeros.");
	return false;
}

// The prologue of the solve entries: `k` arguments, and after them the optional device
bool entry_device(const char *name, Py_ssize_t k, PyObject *const *args, Py_ssize_t nargs, int *device)
{
	if (nargs != k && nargs != k + 1) { PyErr_Format(PyExc_TypeError, "%s requires %zd arguments", name, k); return false; }
	*device = default_device();
	return nargs == k || parse_device(args[k], device);
}

// A failed library call as a Python exception: ValueError for bad arguments, RuntimeError otherwise.  `msg`: the library's
// message of this thread by default.
PyObject *raise_rc(int rc, const char *what, const char *msg = nullptr)
{
	PyErr_Format(rc == GF2BV_ERR_ARG ? PyExc_ValueError : PyExc_RuntimeError, "gf2bv_amd: HIP %s failed (%d): %s", what, rc,
	             msg ? msg : gf2bv_last_error());
	return nullptr;
}

// The digits that can hold bits 0..cols of every equation (sign ignored, higher bits ignored), gathered into ONE
// buffer for the C ABI.  Two phases: offsets + source pointers row by row (type check), then the copy -- into memory
// that is NOT value-initialised first, and by several threads when it is large (the GIL is held by the caller,
// nothing can change the ints; the workers only read): for the 20000 x 19968 recovery systems of the reference's
// examples (53 MB of digits) a zero-filled std::vector plus a single-threaded memcpy were 10 of the 24 ms of a solve.
struct Staging {
	uint32_t *digits = nullptr;
	bool pinned = false;                                       // digits came from gf2bv_host_alloc (page-locked, recycled)
	void drop() { if (pinned) gf2bv_host_free(digits); else free(digits); digits = nullptr; pinned = false; }
	~Staging() { drop(); }
};
struct DigitGather {
	std::vector<int64_t> off = std::vector<int64_t>(1, 0);    // off[r] .. off[r+1]: digits of row r
	std::vector<const uint32_t *> src;                         // first digit of row r
	Staging own;
	uint32_t *digits = nullptr;                                // (gather_list(): every row, in `own`)
	// `src` points into the ints' ob_digit arrays.  m4ri_solve gathers before it first drops the GIL, so borrowed pointers do;
	// m4ri_solve_many gathers chunk k + 1 AFTER it dropped the GIL to wait for chunk k - 1 -- another Python thread may have
	// emptied the caller's lists by then -- and therefore holds a strong reference to every int until the call ends.
	bool hold = false;
	std::vector<PyObject *> held;
	DigitGather() = default;
	DigitGather(const DigitGather &) = delete;
	DigitGather &operator=(const DigitGather &) = delete;
	~DigitGather() { for (PyObject *o : held) Py_DECREF(o); }     // (destroyed by the Python-facing function, GIL held)
	bool add(PyObject *list, Py_ssize_t cols)
	{
		const Py_ssize_t need = (cols + 1 + PyLong_SHIFT - 1) / PyLong_SHIFT;
		const Py_ssize_t rows = PyList_GET_SIZE(list);
		static_assert(sizeof(digit) == sizeof(uint32_t), "30-bit digits in uint32 expected");
		for (Py_ssize_t r = 0; r < rows; r++) {
			PyObject *item = PyList_GET_ITEM(list, r);
			if (!PyLong_Check(item)) {
				PyErr_SetString(PyExc_TypeError, "List items must be integers");
				return false;
			}
			const Py_ssize_t nd = GF2_DIGIT_COUNT((PyLongObject *)item);
			off.push_back(off.back() + (nd < need ? nd : need));
			src.push_back(reinterpret_cast<const uint32_t *>(GF2_DIGITS((PyLongObject *)item)));
			if (hold) { Py_INCREF(item); held.push_back(item); }
		}
		return true;
	}
	// the digits of one list of equations
	bool gather_list(PyObject *list, Py_ssize_t cols)
	{
		const size_t rows = (size_t)PyList_GET_SIZE(list);
		off.reserve(rows + 1); src.reserve(rows);
		if (!add(list, cols) || !gather_rows(0, src.size(), (size_t)1 << 30, own)) return false;
		digits = own.digits;
		return true;
	}
	// Rows r0 .. r1 into a buffer of this object's own (row r's digits at digits + off[r] - off[r0]).  Page-locked staging
	// from the library when the copy is worth a DMA of its own and not larger than pin_max (page-locking more than a call can
	// recycle costs more than the staged copy it saves); no GPU, or no pinned memory left: malloc.
	bool gather_rows(size_t r0, size_t r1, size_t pin_max, Staging &st) const
	{
		st.drop();
		uint32_t *digits = nullptr;
		const int64_t base = off[r0];
		const size_t total = (size_t)(off[r1] - base);
		void *hp = nullptr;
		if ((total + 1) * sizeof(uint32_t) >= (256u << 10) && (total + 1) * sizeof(uint32_t) <= pin_max && gf2bv_host_alloc((int64_t)((total + 1) * sizeof(uint32_t)), &hp) == GF2BV_OK && hp) {
			digits = static_cast<uint32_t *>(hp); st.pinned = true;
		} else digits = static_cast<uint32_t *>(malloc((total + 1) * sizeof(uint32_t)));
		if (!digits) { PyErr_NoMemory(); return false; }
		st.digits = digits;
		auto copy_rows = [this, base, digits](size_t a, size_t b) {
			for (size_t r = a; r < b; r++)
				memcpy(digits + (off[r] - base), src[r], (size_t)(off[r + 1] - off[r]) * sizeof(uint32_t));
		};
		unsigned nt = total * sizeof(uint32_t) >= (8u << 20) ? std::min(8u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
		if (nt <= 1 || r1 - r0 < 64) { copy_rows(r0, r1); return true; }
		// equal shares of the DIGITS, not of the rows
		std::vector<std::thread> th;
		size_t a = r0;
		for (unsigned k = 1; k <= nt; k++) {
			size_t b = r1;
			if (k < nt) {
				const int64_t want = base + (int64_t)(total / nt * k);
				b = (size_t)(std::lower_bound(off.begin() + (ptrdiff_t)r0, off.begin() + (ptrdiff_t)r1 + 1, want) - off.begin());
				if (b > r1) b = r1;
				if (b < a) b = a;
			}
			if (k < nt) th.emplace_back(copy_rows, a, b); else copy_rows(a, b);
			a = b;
		}
		for (auto &t : th) t.join();
		return true;
	}
};

// The prologue of the entries that take one list of equations (m4ri_solve, m4ri_solve_rhs, m4ri_factor): the list and its shape.
// DigitGather::gather_list then collects the digits.
bool parse_equations(PyObject *list, PyObject *cols_obj, PyObject *mode_obj, Py_ssize_t *rows, Py_ssize_t *cols, long *mode)
{
	if (!PyList_Check(list)) {
		PyErr_SetString(PyExc_TypeError, "The first argument equations must be a list");
		return false;
	}
	*rows = PyList_GET_SIZE(list);
	return parse_cols_mode(cols_obj, mode_obj, cols, mode) && rows_cover_cols(*rows, *cols);
}

// The epilogue of the entries that return one result: `call(&res)`, run with the GIL released, is the library call that makes it
// (collect_results below: the entries that return a list)
template <class F>
PyObject *single_result(long mode, int device, F &&call)
{
	gf2bv_result *res = nullptr;
	int rc;
	Py_BEGIN_ALLOW_THREADS          // same place the reference drops the GIL (_internal.c:429)
	rc = call(&res);
	Py_END_ALLOW_THREADS
	if (rc != GF2BV_OK) return raise_rc(rc, "solve");
	return result_to_py(res, mode, device);
}

// ------------------------------------------------------------------------------------------------
// m4ri_solve(equations, cols, mode) -- gf2bv/_internal.c:359-502
PyObject *py_m4ri_solve(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_solve", 3, args, nargs, &device)) return nullptr;
	PyObject *list = args[0];
	Py_ssize_t rows, cols;
	long mode;
	if (!parse_equations(list, args[1], args[2], &rows, &cols, &mode)) return nullptr;
	DigitGather dg;
	if (!dg.gather_list(list, cols)) return nullptr;

	return single_result(mode, device, [&](gf2bv_result **res) {
		return gf2bv_solve_digits(dg.digits, dg.off.data(), PyLong_SHIFT, rows, cols, (int)mode, device, res);
	});
}

// right-hand sides (a list of non-negative ints, bit r = affine term of equation r) -> len(rhs) x ceil(rows / 64) words, bits >= rows
// dropped (m4ri_solve_rhs, Factorization.solve)
bool rhs_list_words(PyObject *rhs, Py_ssize_t rows, std::vector<uint64_t> &words)
{
	const Py_ssize_t nrhs = PyList_GET_SIZE(rhs);
	const int64_t rw = (rows + 63) / 64;
	try { words.assign((size_t)nrhs * (size_t)rw, 0); } catch (const std::bad_alloc &) { PyErr_NoMemory(); return false; }
	PyObject *zero = PyLong_FromLong(0);
	if (!zero) return false;
	for (Py_ssize_t j = 0; j < nrhs; j++) {
		PyObject *item = PyList_GET_ITEM(rhs, j);
		if (!PyLong_Check(item)) { Py_DECREF(zero); PyErr_SetString(PyExc_TypeError, "The right-hand sides must be a list of integers"); return false; }
		const int neg = PyObject_RichCompareBool(item, zero, Py_LT);
		if (neg) Py_DECREF(zero);
		if (neg < 0) return false;
		if (neg) { PyErr_SetString(PyExc_ValueError, "The right-hand sides must be non-negative"); return false; }
		PyLongObject *v = (PyLongObject *)item;
		uint64_t *w = words.data() + (size_t)j * (size_t)rw;
		const Py_ssize_t nd = GF2_DIGIT_COUNT(v);
		for (Py_ssize_t d = 0; d < nd; d++) {
			const int64_t bit = (int64_t)d * PyLong_SHIFT;
			if (bit >= rows) break;
			const uint64_t x = (uint64_t)GF2_DIGITS(v)[d];
			w[bit >> 6] |= x << (bit & 63);
			if ((bit & 63) + PyLong_SHIFT > 64 && (bit >> 6) + 1 < rw) w[(bit >> 6) + 1] |= x >> (64 - (bit & 63));
		}
		if (rows & 63) w[rw - 1] &= ((uint64_t)1 << (rows & 63)) - 1;
	}
	Py_DECREF(zero);
	return true;
}

// result handles -> list of None / int / AffineSpace; frees every handle (also on failure)
PyObject *results_to_list(std::vector<gf2bv_result *> &res, long mode, int device)
{
	const Py_ssize_t n = (Py_ssize_t)res.size();
	PyObject *out = PyList_New(n);
	if (!out) { for (gf2bv_result *r : res) gf2bv_result_free(r); return nullptr; }
	for (Py_ssize_t j = 0; j < n; j++) {
		PyObject *v = result_to_py(res[(size_t)j], mode, device);       // (frees the handle)
		res[(size_t)j] = nullptr;
		if (!v) {
			for (Py_ssize_t k = j + 1; k < n; k++) gf2bv_result_free(res[(size_t)k]);
			Py_DECREF(out);
			return nullptr;
		}
		PyList_SET_ITEM(out, j, v);
	}
	return out;
}

// The epilogue of the list-returning entries: `fill(out)`, run with the GIL released, makes the n result handles of a library call;
// a failure frees whichever exist and raises
template <class F>
PyObject *collect_results(int64_t n, long mode, int device, F &&fill)
{
	std::vector<gf2bv_result *> res((size_t)n, nullptr);
	int rc;
	Py_BEGIN_ALLOW_THREADS
	rc = fill(res.data());
	Py_END_ALLOW_THREADS
	if (rc != GF2BV_OK) {
		for (gf2bv_result *r : res) if (r) gf2bv_result_free(r);
		return raise_rc(rc, "solve");
	}
	return results_to_list(res, mode, device);
}

// ---- what the packed front-ends pass in, one parser per kind of input ---------------------------------------------------------
// The factored form of a system as C-contiguous buffers: lin, then per group of products its offsets and its operands -- four
// buffers for a quadratic system (m4ri_solve_quad_packed's arguments: lin, term_off, ta, tb), eight for a cubic one
// (m4ri_solve_cubic_packed's: lin, off2, ta, tb, off3, ua, ub, uc), thirteen for a quartic one (m4ri_solve_quartic_packed's: the
// cubic eight, then off4, va, vb, vc, vd).  A layout names the groups and words the refusals.
struct TermGroup { int off_at, op_at, arity; };               // argument of the offsets, of the first operand; operands per product
struct TermLayout {
	int nbuf, ngroups;
	TermGroup group[3];
	// The order of the checks, and so which refusal a caller sees for buffers with two faults, is each entry's own from before
	// the parsers were one: the quadratic entries look at the operands' sizes before the offsets' values, the cubic ones behind
	// the offsets' end.  Callers and tests match these texts.
	bool ops_first;
	const char *bad_len, *bad_ops, *bad_start, *bad_end, *bad_order;
};
const TermLayout QUAD_TERMS = {4, 1, {{1, 2, 2}, {0, 0, 0}, {0, 0, 0}}, true,
	"term_off must hold one int64 per row of lin and one more", "ta and tb must hold the same number of whole operands",
	"term_off must start at 0", "term_off must end at the number of operands in ta", "term_off must not decrease"};
const TermLayout CUBIC_TERMS = {8, 2, {{1, 2, 2}, {4, 5, 3}, {0, 0, 0}}, false,
	"off2 and off3 must hold one int64 per row of lin and one more", "the operands of a product must hold the same number of whole forms",
	"off2 and off3 must start at 0", "off2 and off3 must end at the number of operands of their products", "off2 and off3 must not decrease"};
const TermLayout QUARTIC_TERMS = {13, 3, {{1, 2, 2}, {4, 5, 3}, {8, 9, 4}}, false,
	"off2, off3 and off4 must hold one int64 per row of lin and one more", "the operands of a product must hold the same number of whole forms",
	"off2, off3 and off4 must start at 0", "off2, off3 and off4 must end at the number of operands of their products",
	"off2, off3 and off4 must not decrease"};

// The buffers of a layout, checked against each other and against n_lin before the library sees them: whole rows of
// Wl = ceil((n_lin + 1) / 64) words, per group one offset per row and one more, offsets that start at 0, never decrease and end at
// the number of operands, operands of equal size.  TypeError for what is no buffer, ValueError for a shape.
struct TermBuffers {
	const TermLayout &lay;
	Py_buffer view[13];
	int got = 0;
	Py_ssize_t n = 0, live = 0;
	explicit TermBuffers(const TermLayout &layout) : lay(layout) {}
	TermBuffers(const TermBuffers &) = delete;
	TermBuffers &operator=(const TermBuffers &) = delete;
	~TermBuffers() { for (int k = 0; k < got; k++) PyBuffer_Release(&view[k]); }
	const uint64_t *words(int k) const { return static_cast<const uint64_t *>(view[k].buf); }
	const int64_t *offsets(int k) const { return static_cast<const int64_t *>(view[k].buf); }
	bool parse(PyObject *const *args, PyObject *n_obj)
	{
		n = PyLong_AsSsize_t(n_obj);
		if (n == -1 && PyErr_Occurred()) return false;
		if (n < 1 || n > 65535) { PyErr_SetString(PyExc_ValueError, "n_lin must be 1..65535"); return false; }
		const Py_ssize_t wl = (n + 1 + 63) / 64;
		for (; got < lay.nbuf; got++)
			if (PyObject_GetBuffer(args[got], &view[got], PyBUF_C_CONTIGUOUS) != 0) return false;
		live = view[0].len / (wl * 8);
		const char *bad = nullptr;
		if (view[0].len != live * wl * 8) bad = "lin must hold whole rows of ceil((n_lin + 1) / 64) 64-bit words";
		for (int g = 0; g < lay.ngroups && !bad; g++) {
			const TermGroup &tg = lay.group[g];
			const Py_ssize_t nterms = view[tg.op_at].len / (wl * 8);
			const int64_t *off = offsets(tg.off_at);
			bool ops_ok = true;
			for (int k = 0; k < tg.arity; k++) ops_ok = ops_ok && view[tg.op_at + k].len == nterms * wl * 8;
			if (view[tg.off_at].len != (live + 1) * 8) bad = lay.bad_len;
			else if (lay.ops_first && !ops_ok) bad = lay.bad_ops;
			else if (off[0] != 0) bad = lay.bad_start;
			else if (off[live] != nterms) bad = lay.bad_end;
			else if (!ops_ok) bad = lay.bad_ops;
			for (Py_ssize_t r = 0; r < live && !bad; r++)
				if (off[r + 1] < off[r]) bad = lay.bad_order;
		}
		if (bad) { PyErr_SetString(PyExc_ValueError, bad); return false; }
		return true;
	}
	Py_ssize_t cols() const
	{
		const Py_ssize_t c3 = n * (n - 1) * (n - 2) / 6;
		return n + n * (n - 1) / 2 + (lay.ngroups >= 2 ? c3 : 0) + (lay.ngroups == 3 ? (n > 1024 ? (Py_ssize_t)1 << 40 : c3 * (n - 3) / 4) : 0);
	}
};

// (a buffer taken with PyBUF_C_CONTIGUOUS | PyBUF_FORMAT) a 2-D uint64 array?
bool is_u64_matrix(const Py_buffer &view)
{
	const char *f = view.format ? view.format : "B";
	if (*f == '<' || *f == '=' || *f == '@') f++;
	return view.ndim == 2 && view.itemsize == 8 && (strcmp(f, "Q") == 0 || strcmp(f, "L") == 0);
}

// a buffer of the caller's, held until the entry returns
struct HeldBuffer {
	Py_buffer view{};
	bool have = false;
	HeldBuffer() = default;
	HeldBuffer(const HeldBuffer &) = delete;
	HeldBuffer &operator=(const HeldBuffer &) = delete;
	~HeldBuffer() { if (have) PyBuffer_Release(&view); }
	bool take(PyObject *buf, int flags)
	{
		if (PyObject_GetBuffer(buf, &view, flags) != 0) return false;
		return have = true;
	}
};

// rows x words packed equations (m4ri_solve_packed's buffer) as 32-bit digits: two per word
struct PackedRows : HeldBuffer {
	std::vector<int64_t> off;
	bool offsets(Py_ssize_t rows, Py_ssize_t words)
	{
		try { off.resize((size_t)rows + 1); } catch (const std::bad_alloc &) { PyErr_NoMemory(); return false; }
		for (Py_ssize_t r = 0; r <= rows; r++) off[(size_t)r] = (int64_t)r * words * 2;
		return true;
	}
	bool parse(PyObject *buf, Py_ssize_t rows, Py_ssize_t words, Py_ssize_t cols)
	{
		if (!take(buf, PyBUF_C_CONTIGUOUS)) return false;
		if (rows < 0 || words <= 0 || view.len != rows * words * 8 || words * 64 < cols + 1) {
			PyErr_SetString(PyExc_ValueError, "buffer must hold rows x words 64-bit words covering cols + 1 bits");
			return false;
		}
		return offsets(rows, words);
	}
	const uint32_t *digits() const { return static_cast<const uint32_t *>(view.buf); }
};

// right-hand sides, for Factorization.solve and every m4ri_solve_rhs_*packed: a list of non-negative ints or a C-contiguous 2-D
// uint64 array of nrhs x >= ceil(rows / 64) words
struct RhsInput : HeldBuffer {
	std::vector<uint64_t> words;
	const uint64_t *src = nullptr;
	int64_t nrhs = 0, stride = 0;
	bool parse(PyObject *rhs, int64_t rows)
	{
		const int64_t rw = (rows + 63) / 64;
		stride = rw;
		if (PyList_Check(rhs)) {
			nrhs = PyList_GET_SIZE(rhs);
			if (nrhs && !rhs_list_words(rhs, rows, words)) return false;
			src = words.data();
			return true;
		}
		if (!PyObject_CheckBuffer(rhs)) {
			PyErr_SetString(PyExc_TypeError, "The right-hand sides must be a list of integers or a 2-D uint64 array");
			return false;
		}
		if (!take(rhs, PyBUF_C_CONTIGUOUS | PyBUF_FORMAT)) return false;
		if (!is_u64_matrix(view)) {
			PyErr_SetString(PyExc_TypeError, "right-hand sides as a buffer: a C-contiguous 2-D uint64 array");
			return false;
		}
		nrhs = view.shape[0];
		stride = view.shape[1];
		if (stride < rw) {
			PyErr_SetString(PyExc_ValueError, "the right-hand-side array needs ceil(rows / 64) words per row");
			return false;
		}
		src = static_cast<const uint64_t *>(view.buf);
		return true;
	}
};

// The prologue of the entries on m4ri_solve_packed's buffer: arguments 0 .. 4 are the buffer, rows, words, cols and mode
bool parse_packed_call(PyObject *const *args, PackedRows &pr, Py_ssize_t *rows, Py_ssize_t *cols, long *mode)
{
	*rows = PyLong_AsSsize_t(args[1]);
	const Py_ssize_t words = PyLong_AsSsize_t(args[2]);
	if ((*rows == -1 || words == -1) && PyErr_Occurred()) return false;
	return parse_cols_mode(args[3], args[4], cols, mode) && rows_cover_cols(*rows, *cols) && pr.parse(args[0], *rows, words, *cols);
}

// The prologue of the entries that take the factored form and a row count: the first arguments are the layout's buffers, then n_lin,
// rows, mode at the given positions; rows must cover the rows of lin (`live_rows`: the batch entry's systems are checked by its own
// offsets instead) and the columns
bool parse_quad_call(PyObject *const *args, int n_at, int rows_at, int mode_at, bool live_rows, TermBuffers &tb, Py_ssize_t *rows, long *mode)
{
	*rows = PyLong_AsSsize_t(args[rows_at]);
	if (*rows == -1 && PyErr_Occurred()) return false;
	if (!parse_mode(args[mode_at], mode) || !tb.parse(args, args[n_at])) return false;
	if (live_rows && *rows < tb.live) { PyErr_SetString(PyExc_ValueError, "rows must be at least the rows of lin"); return false; }
	return rows_cover_cols(*rows, tb.cols());
}

// m4ri_solve_rhs(equations, cols, mode, rhs, device=None) -> list of (None | int | AffineSpace), one per element of `rhs`.
// New entry (no counterpart in the reference): many systems that share their coefficient matrix -- the reference factors A alone
// (gf2bv/_internal.c:398-433) and only then solves against B (:438-455) -- eliminated ONCE (gf2bv_solve_rhs_digits).  `equations`
// as for m4ri_solve, bit 0 (the affine term) ignored; rhs[j] a non-negative int whose bit r is the affine term of equation r in
// system j (bits >= rows ignored).  Element j is what m4ri_solve returns for `equations` with their affine terms taken from rhs[j].
PyObject *py_m4ri_solve_rhs(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_solve_rhs", 4, args, nargs, &device)) return nullptr;
	PyObject *list = args[0], *rhs = args[3];
	if (!PyList_Check(rhs)) {
		PyErr_SetString(PyExc_TypeError, "The right-hand sides must be a list of integers");
		return nullptr;
	}
	Py_ssize_t rows, cols;
	long mode;
	if (!parse_equations(list, args[1], args[2], &rows, &cols, &mode)) return nullptr;
	const Py_ssize_t nrhs = PyList_GET_SIZE(rhs);
	if (nrhs == 0) return PyList_New(0);
	const int64_t rw = (rows + 63) / 64;
	std::vector<uint64_t> words;
	if (!rhs_list_words(rhs, rows, words)) return nullptr;
	DigitGather dg;
	if (!dg.gather_list(list, cols)) return nullptr;
	return collect_results(nrhs, mode, device, [&](gf2bv_result **out) {
		return gf2bv_solve_rhs_digits(dg.digits, dg.off.data(), PyLong_SHIFT, rows, cols, words.data(), nrhs, rw, (int)mode, device, out);
	});
}

// ---- Factorization: a kept factorization of one matrix (gf2bv_factor_*; no counterpart in the reference) --------------------
// m4ri_factor(equations, cols, mode, device=None) factors the coefficient matrix of `equations` (bit 0 ignored) once; its solve(rhs)
// equals m4ri_solve_rhs(equations, cols, mode, rhs), element for element, for every call.  rhs: a list of non-negative ints (bit r =
// affine term of equation r) or a C-contiguous 2-D uint64 buffer (numpy array) of nrhs x >= ceil(rows / 64) words.
struct FactorObject {
	PyObject_HEAD
	gf2bv_factor *h;                  // nullptr once closed
	int64_t rows, cols;
	long mode;
	int device;
};

PyTypeObject *Factorization_Type;

void factor_dealloc(FactorObject *self)
{
	PyTypeObject *tp = Py_TYPE(self);
	if (self->h) {
		gf2bv_factor *h = self->h;
		self->h = nullptr;
		Py_BEGIN_ALLOW_THREADS
		gf2bv_factor_free(h);
		Py_END_ALLOW_THREADS
	}
	tp->tp_free((PyObject *)self);
	Py_DECREF(tp);
}

bool factor_open(FactorObject *self)
{
	if (self->h) return true;
	PyErr_SetString(PyExc_ValueError, "the factorization is closed");
	return false;
}

// The library's getters take the handle's mutex, which an append or a solve on another thread holds for its whole run: the GIL is
// dropped around them like around every other call, so that the wait stalls this thread alone.
template <class F>
int64_t factor_get(gf2bv_factor *h, F &&get)
{
	int64_t v;
	Py_BEGIN_ALLOW_THREADS
	v = get(h);
	Py_END_ALLOW_THREADS
	return v;
}

PyObject *factor_rank(FactorObject *self, void *)
{
	return factor_open(self) ? PyLong_FromLongLong(factor_get(self->h, [](gf2bv_factor *h) { return gf2bv_factor_rank(h); })) : nullptr;
}
PyObject *factor_rows(FactorObject *self, void *) { return PyLong_FromLongLong(self->rows); }
PyObject *factor_cols(FactorObject *self, void *) { return PyLong_FromLongLong(self->cols); }
PyObject *factor_mode(FactorObject *self, void *) { return PyLong_FromLong(self->mode); }
PyObject *factor_device(FactorObject *self, void *) { return PyLong_FromLong(self->device); }
PyObject *factor_device_bytes(FactorObject *self, void *)
{
	return factor_open(self) ? PyLong_FromLongLong(factor_get(self->h, [](gf2bv_factor *h) { return gf2bv_factor_device_bytes(h); })) : nullptr;
}
// ONE locked call into a buffer of cols entries pre-filled with -1: an append on another thread may raise the rank between two calls,
// so the count comes from what was written, and (count, pivots) is a state the handle really was in
PyObject *factor_pivots(FactorObject *self, void *)
{
	if (!factor_open(self)) return nullptr;
	std::vector<int32_t> piv((size_t)std::max<int64_t>(1, self->cols), -1);
	int32_t *out = piv.data();
	const int64_t rc = factor_get(self->h, [out](gf2bv_factor *h) { return (int64_t)gf2bv_factor_pivots(h, out); });
	if (rc != GF2BV_OK) return raise_rc((int)rc, "pivots");
	int64_t rank = 0;
	while (rank < (int64_t)piv.size() && piv[(size_t)rank] >= 0) rank++;
	PyObject *t = PyTuple_New(rank);
	if (!t) return nullptr;
	for (int64_t i = 0; i < rank; i++) {
		PyObject *v = PyLong_FromLong(piv[(size_t)i]);
		if (!v) { Py_DECREF(t); return nullptr; }
		PyTuple_SET_ITEM(t, i, v);
	}
	return t;
}

PyObject *new_factorization(gf2bv_factor *h, int64_t rows, int64_t cols, long mode, int device)
{
	FactorObject *f = PyObject_New(FactorObject, Factorization_Type);
	if (!f) { gf2bv_factor_free(h); return nullptr; }
	f->h = h; f->rows = rows; f->cols = cols; f->mode = mode; f->device = device;
	return (PyObject *)f;
}

// The epilogue of the entries that return a Factorization, the twin of single_result: `call(&h)` factors a matrix of rows x cols
template <class F>
PyObject *factor_result(int64_t rows, int64_t cols, long mode, int device, F &&call)
{
	gf2bv_factor *h = nullptr;
	int rc;
	Py_BEGIN_ALLOW_THREADS
	rc = call(&h);
	Py_END_ALLOW_THREADS
	if (rc != GF2BV_OK) return raise_rc(rc, "factorization");
	return new_factorization(h, rows, cols, mode, device);
}

PyObject *factor_solve(FactorObject *self, PyObject *rhs)
{
	if (!factor_open(self)) return nullptr;
	RhsInput ri;
	if (!ri.parse(rhs, self->rows)) return nullptr;
	if (ri.nrhs == 0) return PyList_New(0);
	gf2bv_factor *h = self->h;
	return collect_results(ri.nrhs, self->mode, self->device, [&](gf2bv_result **out) { return gf2bv_factor_solve(h, ri.src, ri.nrhs, ri.stride, out); });
}

// append(equations): equations added below the factored ones -- a list of equation ints (bit 0 ignored) or a C-contiguous 2-D
// uint64 array of n x words words in the same bit order (m4ri_solve_packed's layout); the handle then stands for the stacked matrix
PyObject *factor_append(FactorObject *self, PyObject *eqs)
{
	if (!factor_open(self)) return nullptr;
	int rc;
	gf2bv_factor *h = self->h;
	if (PyList_Check(eqs)) {
		const int64_t n = PyList_GET_SIZE(eqs);
		if (n == 0) Py_RETURN_NONE;
		DigitGather dg;
		if (!dg.gather_list(eqs, self->cols)) return nullptr;
		Py_BEGIN_ALLOW_THREADS
		rc = gf2bv_factor_append_digits(h, dg.digits, dg.off.data(), PyLong_SHIFT, n);
		Py_END_ALLOW_THREADS
	} else if (PyObject_CheckBuffer(eqs)) {
		PackedRows pr;
		if (!pr.take(eqs, PyBUF_C_CONTIGUOUS | PyBUF_FORMAT)) return nullptr;
		if (!is_u64_matrix(pr.view)) {
			PyErr_SetString(PyExc_TypeError, "equations as a buffer: a C-contiguous 2-D uint64 array");
			return nullptr;
		}
		const int64_t n = pr.view.shape[0], words = pr.view.shape[1];
		if (words * 64 < self->cols + 1) {
			PyErr_SetString(PyExc_ValueError, "the equation array needs words covering cols + 1 bits");
			return nullptr;
		}
		if (n == 0) Py_RETURN_NONE;
		if (!pr.offsets(n, words)) return nullptr;
		Py_BEGIN_ALLOW_THREADS
		rc = gf2bv_factor_append_digits(h, pr.digits(), pr.off.data(), 32, n);
		Py_END_ALLOW_THREADS
	} else {
		PyErr_SetString(PyExc_TypeError, "The equations must be a list of integers or a 2-D uint64 array");
		return nullptr;
	}
	if (rc != GF2BV_OK) return raise_rc(rc, "append");
	self->rows = gf2bv_factor_rows(h);
	Py_RETURN_NONE;
}

// append_quad(lin, term_off, ta, tb, n_lin): factored quadratic equations (m4ri_factor_quad_packed's arrays) added below the factored
// ones, expanded on the device (gf2bv_factor_append_quad_terms); n_lin must be the one the factorization was made with
PyObject *factor_append_quad(FactorObject *self, PyObject *const *args, Py_ssize_t nargs)
{
	if (nargs != 5) { PyErr_SetString(PyExc_TypeError, "append_quad requires 5 arguments"); return nullptr; }
	if (!factor_open(self)) return nullptr;
	TermBuffers qb(QUAD_TERMS);
	if (!qb.parse(args, args[4])) return nullptr;
	if (qb.cols() != self->cols) { PyErr_SetString(PyExc_ValueError, "n_lin does not match the factorization's columns"); return nullptr; }
	if (qb.live == 0) Py_RETURN_NONE;
	gf2bv_factor *h = self->h;
	int rc;
	Py_BEGIN_ALLOW_THREADS
	rc = gf2bv_factor_append_quad_terms(h, qb.words(0), qb.offsets(1), qb.words(2), qb.words(3), qb.live, qb.n);
	Py_END_ALLOW_THREADS
	if (rc != GF2BV_OK) return raise_rc(rc, "append");
	self->rows = gf2bv_factor_rows(h);
	Py_RETURN_NONE;
}

// copy(): an independent Factorization with the same state (a device-to-device copy)
PyObject *factor_copy(FactorObject *self, PyObject *)
{
	if (!factor_open(self)) return nullptr;
	gf2bv_factor *h = self->h, *c = nullptr;
	int rc;
	Py_BEGIN_ALLOW_THREADS
	rc = gf2bv_factor_copy(h, &c);
	Py_END_ALLOW_THREADS
	if (rc != GF2BV_OK) return raise_rc(rc, "copy");
	return new_factorization(c, self->rows, self->cols, self->mode, self->device);
}

PyObject *factor_close(FactorObject *self, PyObject *)
{
	if (self->h) {
		gf2bv_factor *h = self->h;
		self->h = nullptr;
		Py_BEGIN_ALLOW_THREADS
		gf2bv_factor_free(h);
		Py_END_ALLOW_THREADS
	}
	Py_RETURN_NONE;
}

PyObject *factor_enter(FactorObject *self, PyObject *)
{
	if (!factor_open(self)) return nullptr;
	Py_INCREF(self);
	return (PyObject *)self;
}

PyObject *factor_exit(FactorObject *self, PyObject *const *, Py_ssize_t) { return factor_close(self, nullptr); }

PyGetSetDef factor_getset[] = {
	{"rank", (getter)factor_rank, nullptr, "rank of the coefficient matrix", nullptr},
	{"pivots", (getter)factor_pivots, nullptr, "pivot columns (the column rank profile), a tuple", nullptr},
	{"rows", (getter)factor_rows, nullptr, "equations (the factored ones plus every appended one)", nullptr},
	{"cols", (getter)factor_cols, nullptr, "unknowns", nullptr},
	{"mode", (getter)factor_mode, nullptr, "0: solve returns ints, 1: AffineSpace objects", nullptr},
	{"device", (getter)factor_device, nullptr, "GPU that holds the factorization", nullptr},
	{"device_bytes", (getter)factor_device_bytes, nullptr, "device memory the factorization holds", nullptr},
	{nullptr, nullptr, nullptr, nullptr, nullptr}};

PyMethodDef factor_methods[] = {
	{"solve", (PyCFunction)factor_solve, METH_O,
	 "solve(rhs)\n--\n\nOne m4ri_solve result per right-hand side (a list of ints, bit r = affine term of equation r, or an nrhs x words uint64 array)."},
	{"append", (PyCFunction)factor_append, METH_O,
	 "append(equations)\n--\n\nAdd equations (a list of ints, bit 0 ignored, or an n x words uint64 array in the same bit order) below the factored ones; later solves take ceil(rows / 64)-word right-hand sides of the stacked system."},
	{"append_quad", (PyCFunction)(void (*)(void))factor_append_quad, METH_FASTCALL,
	 "append_quad(lin, term_off, ta, tb, n_lin)\n--\n\nAdd factored quadratic equations (m4ri_factor_quad_packed's arrays) below the factored ones; they are expanded on the device."},
	{"copy", (PyCFunction)factor_copy, METH_NOARGS, "copy()\n--\n\nAn independent Factorization with the same state (a device-to-device copy, no factorization)."},
	{"close", (PyCFunction)factor_close, METH_NOARGS, "close()\n--\n\nRelease the device memory; later use raises ValueError."},
	{"__enter__", (PyCFunction)factor_enter, METH_NOARGS, nullptr},
	{"__exit__", (PyCFunction)(void (*)(void))factor_exit, METH_FASTCALL, nullptr},
	{nullptr, nullptr, 0, nullptr}};

PyType_Slot factor_slots[] = {
	{Py_tp_dealloc, (void *)factor_dealloc}, {Py_tp_methods, (void *)factor_methods}, {Py_tp_getset, (void *)factor_getset}, {0, nullptr}};
PyType_Spec factor_spec = {"_internal.Factorization", sizeof(FactorObject), 0,
                           Py_TPFLAGS_DEFAULT | Py_TPFLAGS_DISALLOW_INSTANTIATION, factor_slots};

PyObject *py_m4ri_factor(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_factor", 3, args, nargs, &device)) return nullptr;
	PyObject *list = args[0];
	Py_ssize_t rows, cols;
	long mode;
	if (!parse_equations(list, args[1], args[2], &rows, &cols, &mode)) return nullptr;
	DigitGather dg;
	if (!dg.gather_list(list, cols)) return nullptr;
	return factor_result(rows, cols, mode, device, [&](gf2bv_factor **h) {
		return gf2bv_factor_digits(dg.digits, dg.off.data(), PyLong_SHIFT, rows, cols, (int)mode, device, h);
	});
}

// m4ri_solve_packed(buffer, rows, words, cols, mode) -> None | int | AffineSpace.
// New entry: the equations arrive ALREADY PACKED -- `rows` x `words` little-endian 64-bit words in the
// bit order of the equation ints (bit 0 = affine term, bit k = coefficient of variable k-1), e.g. the numpy array a
// PackedLinearSystem builds -- instead of as a list of Python ints.  No PyLong is created or read: the buffer goes
// to gf2bv_solve_digits as 32-bit "digits" and the device pack kernel (k_pack_digits) does what
// gf2bv/_internal.c:403-426 does bit by bit.  Same checks, same result types as m4ri_solve.
PyObject *py_m4ri_solve_packed(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_solve_packed", 5, args, nargs, &device)) return nullptr;
	Py_ssize_t rows, cols;
	long mode;
	PackedRows pr;
	if (!parse_packed_call(args, pr, &rows, &cols, &mode)) return nullptr;
	return single_result(mode, device, [&](gf2bv_result **res) {
		return gf2bv_solve_digits(pr.digits(), pr.off.data(), 32, rows, cols, (int)mode, device, res);
	});
}

// m4ri_solve_quad_packed(lin, term_off, ta, tb, n_lin, rows, mode[, device]) -> None | int | AffineSpace.
// New entry (no counterpart in the reference): a quadratic system kept FACTORED -- per equation a linear form and products of two
// linear forms over the n_lin + 1 bits of the unlinearised unknowns (gf2bv_hip.h, "quadratic expansion") -- is expanded into the
// linearised matrix on the device and solved there; no equation int over the n_lin(n_lin-1)/2 product unknowns exists on the host.
// lin: rows_live x Wl 64-bit words, term_off: rows_live + 1 int64, ta / tb: term_off[-1] x Wl words each (C-contiguous buffers,
// Wl = ceil((n_lin + 1) / 64)); rows >= rows_live: the row count the solver sees (zero rows are added on the device).  Same result
// types as m4ri_solve over n_lin + n_lin(n_lin-1)/2 columns.
PyObject *py_m4ri_solve_quad_packed(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_solve_quad_packed", 7, args, nargs, &device)) return nullptr;
	Py_ssize_t rows;
	long mode;
	TermBuffers qb(QUAD_TERMS);
	if (!parse_quad_call(args, 4, 5, 6, true, qb, &rows, &mode)) return nullptr;
	return single_result(mode, device, [&](gf2bv_result **res) {
		return gf2bv_solve_quad_terms(qb.words(0), qb.offsets(1), qb.words(2), qb.words(3), qb.live, rows, qb.n, (int)mode, device, res);
	});
}

// m4ri_solve_cubic_packed(lin, off2, ta, tb, off3, ua, ub, uc, n_lin, rows, mode[, device]) -> None | int | AffineSpace.
// New entry (no counterpart in the reference): a cubic system kept FACTORED -- per equation a linear form, products of two and
// products of three affine forms over the n_lin + 1 bits of the unknowns, the products exact (gf2bv_hip.h, "cubic expansion") -- is
// expanded over the n_lin + C(n_lin,2) + C(n_lin,3) columns on the device and solved there.  Buffers as for m4ri_solve_quad_packed,
// off3 / ua / ub / uc the cubic twins of off2 / ta / tb; rows >= the rows of lin and >= the columns.
PyObject *py_m4ri_solve_cubic_packed(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_solve_cubic_packed", 11, args, nargs, &device)) return nullptr;
	Py_ssize_t rows;
	long mode;
	TermBuffers cb(CUBIC_TERMS);
	if (!parse_quad_call(args, 8, 9, 10, true, cb, &rows, &mode)) return nullptr;
	return single_result(mode, device, [&](gf2bv_result **res) {
		return gf2bv_solve_cubic_terms(cb.words(0), cb.offsets(1), cb.words(2), cb.words(3), cb.offsets(4), cb.words(5), cb.words(6), cb.words(7),
		                               cb.live, rows, cb.n, (int)mode, device, res);
	});
}

// m4ri_solve_quartic_packed(lin, off2, ta, tb, off3, ua, ub, uc, off4, va, vb, vc, vd, n_lin, rows, mode[, device]) -> None | int |
// AffineSpace.  New entry (no counterpart in the reference): m4ri_solve_cubic_packed one arity up -- products of four affine forms too
// (off4 / va / vb / vc / vd), expanded over the n_lin + C(n_lin,2) + C(n_lin,3) + C(n_lin,4) columns on the device
// (gf2bv_hip.h, "quartic expansion") and solved there; rows >= the rows of lin and >= the columns.
PyObject *py_m4ri_solve_quartic_packed(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_solve_quartic_packed", 16, args, nargs, &device)) return nullptr;
	Py_ssize_t rows;
	long mode;
	TermBuffers qb(QUARTIC_TERMS);
	if (!parse_quad_call(args, 13, 14, 15, true, qb, &rows, &mode)) return nullptr;
	return single_result(mode, device, [&](gf2bv_result **res) {
		return gf2bv_solve_quartic_terms(qb.words(0), qb.offsets(1), qb.words(2), qb.words(3), qb.offsets(4), qb.words(5), qb.words(6), qb.words(7),
		                                 qb.offsets(8), qb.words(9), qb.words(10), qb.words(11), qb.words(12), qb.live, rows, qb.n, (int)mode,
		                                 device, res);
	});
}

// m4ri_solve_xl4_cubic_packed(lin, off2, ta, tb, off3, ua, ub, uc, n_lin, mode[, device]) -> None | int | AffineSpace over the
// n_lin + C(n_lin,2) + C(n_lin,3) + C(n_lin,4) columns of degree-4 XL.  New entry (no counterpart in the reference):
// m4ri_solve_cubic_packed's arrays (every row live), expanded, multiplied by 1 and by every unknown, padded and solved on the device
// (gf2bv_solve_xl4_cubic_terms; gf2bv_hip.h, "degree-4 XL on cubic equations")
PyObject *py_m4ri_solve_xl4_cubic_packed(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_solve_xl4_cubic_packed", 10, args, nargs, &device)) return nullptr;
	long mode;
	TermBuffers cb(CUBIC_TERMS);
	if (!parse_mode(args[9], &mode) || !cb.parse(args, args[8])) return nullptr;
	return single_result(mode, device, [&](gf2bv_result **res) {
		return gf2bv_solve_xl4_cubic_terms(cb.words(0), cb.offsets(1), cb.words(2), cb.words(3), cb.offsets(4), cb.words(5), cb.words(6), cb.words(7),
		                                   cb.live, cb.n, (int)mode, device, res);
	});
}

// ---- degree-3 XL: quadratic equations multiplied by 1 and by every unknown on the device (gf2bv_hip.h, "degree-3 XL") --------------
// (every entry of this section and of the hybrid one is a template over the degree D: m4ri_solve_xl4* are the same code on the xl4
// entries of the library, over the monomials of degree <= 4 -- gf2bv_hip.h, "degree-4 XL")
// QuadraticSystem's equation ints of `list` as augmented words over the n_lin = `n_obj` unknowns and their pairs (column c = bit 1 + c,
// the constant at column cols2), w2 words a row: one pass over the digits
bool quad_rows_from_ints(PyObject *list, PyObject *n_obj, std::vector<uint64_t> &quad, int64_t *m_out, int64_t *n_out, int64_t *w2_out)
{
	if (!PyList_Check(list)) { PyErr_SetString(PyExc_TypeError, "The first argument equations must be a list"); return false; }
	const Py_ssize_t n = PyLong_AsSsize_t(n_obj);
	if (n == -1 && PyErr_Occurred()) return false;
	if (n < 1 || n > 65535) { PyErr_SetString(PyExc_ValueError, "n_lin must be 1..65535"); return false; }
	const int64_t m = PyList_GET_SIZE(list), cols2 = n + n * (n - 1) / 2, w2 = (cols2 + 1 + 63) / 64;
	try { quad.assign((size_t)(m * w2), 0); } catch (const std::bad_alloc &) { PyErr_NoMemory(); return false; }
	for (int64_t r = 0; r < m; r++) {
		PyObject *item = PyList_GET_ITEM(list, r);
		if (!PyLong_Check(item)) { PyErr_SetString(PyExc_TypeError, "List items must be integers"); return false; }
		PyLongObject *v = (PyLongObject *)item;
		uint64_t *w = quad.data() + (size_t)(r * w2);
		const Py_ssize_t nd = GF2_DIGIT_COUNT(v);
		for (Py_ssize_t d = 0; d < nd; d++) {                      // bit b of the int is column b - 1
			uint64_t x = (uint64_t)GF2_DIGITS(v)[d];
			int64_t at = (int64_t)d * PyLong_SHIFT - 1;
			if (d == 0) { x >>= 1; at = 0; }
			if (at >= cols2) break;
			w[at >> 6] |= x << (at & 63);
			if ((at & 63) + PyLong_SHIFT > 64 && (at >> 6) + 1 < w2) w[(at >> 6) + 1] |= x >> (64 - (at & 63));
		}
		for (int64_t k = (cols2 >> 6) + 1; k < w2; k++) w[k] = 0;  // (nothing above the columns)
		w[cols2 >> 6] &= ((uint64_t)1 << (cols2 & 63)) - 1;
		if (nd > 0 && (GF2_DIGITS(v)[0] & 1)) w[cols2 >> 6] |= (uint64_t)1 << (cols2 & 63);      // the constant: column cols2
	}
	*m_out = m; *n_out = n; *w2_out = w2;
	return true;
}

// m4ri_solve_xl3(equations, n_lin, mode[, device]) -> None | int | AffineSpace over n_lin + C(n_lin,2) + C(n_lin,3) columns.
// New entry (no counterpart in the reference): `equations` are QuadraticSystem's equation ints (bit 0 the constant, bit 1 + c column
// c of the n_lin + C(n_lin,2) linearised unknowns; higher bits and the sign ignored).  They are written as augmented words on the
// host -- one pass over the digits, no PyLong is made -- and gf2bv_solve_xl3_words multiplies, pads and solves them on the device.
template <int D> PyObject *py_m4ri_solve_xl(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device(D == 4 ? "m4ri_solve_xl4" : "m4ri_solve_xl3", 3, args, nargs, &device)) return nullptr;
	long mode;
	if (!parse_mode(args[2], &mode)) return nullptr;
	std::vector<uint64_t> quad;
	int64_t m, n, w2;
	if (!quad_rows_from_ints(args[0], args[1], quad, &m, &n, &w2)) return nullptr;
	return single_result(mode, device, [&](gf2bv_result **res) {
		return (D == 4 ? gf2bv_solve_xl4_words : gf2bv_solve_xl3_words)(quad.data(), m, w2, n, (int)mode, device, res);
	});
}

// m4ri_solve_xl3_quad_packed(lin, term_off, ta, tb, n_lin, mode[, device]) -> None | int | AffineSpace: m4ri_solve_quad_packed's
// arrays (every row live), expanded, multiplied, padded and solved on the device (gf2bv_solve_xl3_quad_terms)
template <int D> PyObject *py_m4ri_solve_xl_quad_packed(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device(D == 4 ? "m4ri_solve_xl4_quad_packed" : "m4ri_solve_xl3_quad_packed", 6, args, nargs, &device)) return nullptr;
	long mode;
	TermBuffers qb(QUAD_TERMS);
	if (!parse_mode(args[5], &mode) || !qb.parse(args, args[4])) return nullptr;
	return single_result(mode, device, [&](gf2bv_result **res) {
		return (D == 4 ? gf2bv_solve_xl4_quad_terms : gf2bv_solve_xl3_quad_terms)(qb.words(0), qb.offsets(1), qb.words(2), qb.words(3), qb.live, qb.n, (int)mode, device, res);
	});
}

// ---- hybrid XL: guessed unknowns, every assignment's system in one batch (gf2bv_hip.h, "hybrid XL") ---------------------------------
// (guess, a0, na) of the two entries below: a sequence of unknown indices and the range of assignments; the library checks the values
struct GuessArgs {
	std::vector<int32_t> g;
	int64_t a0 = 0, na = 0;
	bool parse(PyObject *guess, PyObject *a0_obj, PyObject *na_obj)
	{
		PyObject *seq = PySequence_Fast(guess, "guess must be a sequence of unknown indices");
		if (!seq) return false;
		const Py_ssize_t f = PySequence_Fast_GET_SIZE(seq);
		bool ok = true;
		for (Py_ssize_t t = 0; t < f && ok; t++) {
			const long v = PyLong_AsLong(PySequence_Fast_GET_ITEM(seq, t));
			if (v == -1 && PyErr_Occurred()) ok = false;
			else if (v < 0 || v > 65535) { PyErr_SetString(PyExc_ValueError, "a guessed unknown must be 0 .. n_lin - 1"); ok = false; }
			else g.push_back((int32_t)v);
		}
		Py_DECREF(seq);
		if (!ok) return false;
		a0 = PyLong_AsLongLong(a0_obj);
		if (a0 == -1 && PyErr_Occurred()) return false;
		na = PyLong_AsLongLong(na_obj);
		if (na == -1 && PyErr_Occurred()) return false;
		if (a0 < 0 || na < 0 || na >= ((int64_t)1 << 31)) { PyErr_SetString(PyExc_ValueError, "the assignments must be a range of 0 .. 2^nguess - 1"); return false; }
		return true;
	}
};

// m4ri_solve_xl3_guess(equations, n_lin, guess, a0, na, mode[, device]) -> list of None | int | AffineSpace over the cubic columns of
// the n_lin - len(guess) remaining unknowns, element s for assignment a0 + s (bit t of it the value of unknown guess[t]).
// New entry (no counterpart in the reference): the equation ints are written as augmented words in one pass, as m4ri_solve_xl3 does,
// and gf2bv_solve_xl3_guess_words substitutes, multiplies, pads and solves every assignment's system on the device as one batch.
template <int D> PyObject *py_m4ri_solve_xl_guess(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device(D == 4 ? "m4ri_solve_xl4_guess" : "m4ri_solve_xl3_guess", 6, args, nargs, &device)) return nullptr;
	long mode;
	GuessArgs ga;
	if (!parse_mode(args[5], &mode) || !ga.parse(args[2], args[3], args[4])) return nullptr;
	std::vector<uint64_t> quad;
	int64_t m, n, w2;
	if (!quad_rows_from_ints(args[0], args[1], quad, &m, &n, &w2)) return nullptr;
	if (ga.na == 0) return PyList_New(0);
	return collect_results(ga.na, mode, device, [&](gf2bv_result **out) {
		return (D == 4 ? gf2bv_solve_xl4_guess_words : gf2bv_solve_xl3_guess_words)(quad.data(), m, w2, n, ga.g.data(), (int64_t)ga.g.size(), ga.a0, ga.na, (int)mode, device, out);
	});
}

// m4ri_solve_xl3_guess_quad_packed(lin, term_off, ta, tb, n_lin, guess, a0, na, mode[, device]) -> list: m4ri_solve_xl3_guess on
// m4ri_solve_quad_packed's arrays (every row live), expanded on the device first (gf2bv_solve_xl3_guess_quad_terms)
template <int D> PyObject *py_m4ri_solve_xl_guess_quad_packed(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device(D == 4 ? "m4ri_solve_xl4_guess_quad_packed" : "m4ri_solve_xl3_guess_quad_packed", 9, args, nargs, &device)) return nullptr;
	long mode;
	GuessArgs ga;
	TermBuffers qb(QUAD_TERMS);
	if (!parse_mode(args[8], &mode) || !ga.parse(args[5], args[6], args[7]) || !qb.parse(args, args[4])) return nullptr;
	if (ga.na == 0) return PyList_New(0);
	return collect_results(ga.na, mode, device, [&](gf2bv_result **out) {
		return (D == 4 ? gf2bv_solve_xl4_guess_quad_terms : gf2bv_solve_xl3_guess_quad_terms)(qb.words(0), qb.offsets(1), qb.words(2), qb.words(3), qb.live, qb.n, ga.g.data(),
		                                                                                     (int64_t)ga.g.size(), ga.a0, ga.na, (int)mode, device, out);
	});
}

// m4ri_solve_xl4_guess_cubic_packed(lin, off2, ta, tb, off3, ua, ub, uc, n_lin, guess, a0, na, mode[, device]) -> list of None | int |
// AffineSpace over the quartic columns of the n_lin - len(guess) remaining unknowns, element s for assignment a0 + s: hybrid degree-4
// XL on m4ri_solve_cubic_packed's arrays (every row live), expanded, specialised, multiplied and solved on the device as one batch
// (gf2bv_solve_xl4_cubic_guess_terms; gf2bv_hip.h, "hybrid degree-4 XL on cubic equations")
PyObject *py_m4ri_solve_xl4_guess_cubic_packed(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_solve_xl4_guess_cubic_packed", 13, args, nargs, &device)) return nullptr;
	long mode;
	GuessArgs ga;
	TermBuffers cb(CUBIC_TERMS);
	if (!parse_mode(args[12], &mode) || !ga.parse(args[9], args[10], args[11]) || !cb.parse(args, args[8])) return nullptr;
	if (ga.na == 0) return PyList_New(0);
	return collect_results(ga.na, mode, device, [&](gf2bv_result **out) {
		return gf2bv_solve_xl4_cubic_guess_terms(cb.words(0), cb.offsets(1), cb.words(2), cb.words(3), cb.offsets(4), cb.words(5), cb.words(6),
		                                         cb.words(7), cb.live, cb.n, ga.g.data(), (int64_t)ga.g.size(), ga.a0, ga.na, (int)mode, device, out);
	});
}

// ---- the packed front-ends in front of the kept factorization, the shared elimination and the batch --------------------------
// m4ri_factor_packed(buffer, rows, words, cols, mode[, device]) -> Factorization: m4ri_factor on m4ri_solve_packed's buffer
// (gf2bv_factor_digits, 32 payload bits per digit)
PyObject *py_m4ri_factor_packed(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_factor_packed", 5, args, nargs, &device)) return nullptr;
	Py_ssize_t rows, cols;
	long mode;
	PackedRows pr;
	if (!parse_packed_call(args, pr, &rows, &cols, &mode)) return nullptr;
	return factor_result(rows, cols, mode, device, [&](gf2bv_factor **h) {
		return gf2bv_factor_digits(pr.digits(), pr.off.data(), 32, rows, cols, (int)mode, device, h);
	});
}

// m4ri_factor_quad_packed(lin, term_off, ta, tb, n_lin, rows, mode[, device]) -> Factorization over n_lin + n_lin(n_lin-1)/2
// columns: m4ri_solve_quad_packed's arguments, expanded on the device and factored there (gf2bv_factor_quad_terms)
PyObject *py_m4ri_factor_quad_packed(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_factor_quad_packed", 7, args, nargs, &device)) return nullptr;
	Py_ssize_t rows;
	long mode;
	TermBuffers qb(QUAD_TERMS);
	if (!parse_quad_call(args, 4, 5, 6, true, qb, &rows, &mode)) return nullptr;
	return factor_result(rows, qb.cols(), mode, device, [&](gf2bv_factor **h) {
		return gf2bv_factor_quad_terms(qb.words(0), qb.offsets(1), qb.words(2), qb.words(3), qb.live, rows, qb.n, (int)mode, device, h);
	});
}

// m4ri_solve_rhs_packed(buffer, rows, words, cols, mode, rhs[, device]) -> list: m4ri_solve_rhs on m4ri_solve_packed's buffer;
// rhs as Factorization.solve takes it
PyObject *py_m4ri_solve_rhs_packed(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_solve_rhs_packed", 6, args, nargs, &device)) return nullptr;
	Py_ssize_t rows, cols;
	long mode;
	PackedRows pr;
	if (!parse_packed_call(args, pr, &rows, &cols, &mode)) return nullptr;
	RhsInput ri;
	if (!ri.parse(args[5], rows)) return nullptr;
	if (ri.nrhs == 0) return PyList_New(0);
	return collect_results(ri.nrhs, mode, device, [&](gf2bv_result **out) {
		return gf2bv_solve_rhs_digits(pr.digits(), pr.off.data(), 32, rows, cols, ri.src, ri.nrhs, ri.stride, (int)mode, device, out);
	});
}

// m4ri_solve_rhs_quad_packed(lin, term_off, ta, tb, n_lin, rows, mode, rhs[, device]) -> list: one elimination of the expanded
// system for every right-hand side (gf2bv_solve_rhs_quad_terms); the constants of the factored rows are NOT read, rhs holds them
PyObject *py_m4ri_solve_rhs_quad_packed(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_solve_rhs_quad_packed", 8, args, nargs, &device)) return nullptr;
	Py_ssize_t rows;
	long mode;
	TermBuffers qb(QUAD_TERMS);
	if (!parse_quad_call(args, 4, 5, 6, true, qb, &rows, &mode)) return nullptr;
	RhsInput ri;
	if (!ri.parse(args[7], rows)) return nullptr;
	if (ri.nrhs == 0) return PyList_New(0);
	return collect_results(ri.nrhs, mode, device, [&](gf2bv_result **out) {
		return gf2bv_solve_rhs_quad_terms(qb.words(0), qb.offsets(1), qb.words(2), qb.words(3), qb.live, rows, qb.n, ri.src, ri.nrhs, ri.stride, (int)mode, device, out);
	});
}

// m4ri_solve_many_quad_packed(lin, term_off, ta, tb, sys_row_off, n_lin, rows, mode[, device]) -> list, one element per system:
// independent quadratic systems over the same n_lin as one concatenated term set, system s the rows sys_row_off[s] ..
// sys_row_off[s + 1] (a C-contiguous int64 buffer of nsys + 1 offsets from 0), each padded to `rows` rows on the device and all
// solved as lock-step gangs (gf2bv_solve_batch_quad_terms); element s is what m4ri_solve_quad_packed returns for system s
PyObject *py_m4ri_solve_many_quad_packed(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_solve_many_quad_packed", 8, args, nargs, &device)) return nullptr;
	Py_ssize_t rows;
	long mode;
	TermBuffers qb(QUAD_TERMS);
	if (!parse_quad_call(args, 5, 6, 7, false, qb, &rows, &mode)) return nullptr;
	HeldBuffer sv;
	if (!sv.take(args[4], PyBUF_C_CONTIGUOUS)) return nullptr;
	const int64_t *sys = static_cast<const int64_t *>(sv.view.buf);
	const Py_ssize_t nsys = sv.view.len / 8 - 1;
	const char *bad = nullptr;
	if (sv.view.len % 8 || nsys < 0) bad = "sys_row_off must hold one int64 per system and one more";
	else if (sys[0] != 0) bad = "sys_row_off must start at 0";
	else if (sys[nsys] != qb.live) bad = "sys_row_off must end at the rows of lin";
	else
		for (Py_ssize_t k = 0; k < nsys; k++) {
			if (sys[k + 1] < sys[k]) { bad = "sys_row_off must not decrease"; break; }
			if (sys[k + 1] - sys[k] > rows) { bad = "rows must be at least the rows of every system"; break; }
		}
	if (bad) { PyErr_SetString(PyExc_ValueError, bad); return nullptr; }
	if (nsys == 0) return PyList_New(0);
	return collect_results(nsys, mode, device, [&](gf2bv_result **out) {
		return gf2bv_solve_batch_quad_terms(qb.words(0), qb.offsets(1), qb.words(2), qb.words(3), sys, nsys, rows, qb.n, (int)mode, device, out);
	});
}

// m4ri_solve_many(list_of_equation_lists, cols, mode[, devices]) -> list of (None | int | AffineSpace).
// New entry (no counterpart in the reference): independent systems of one shape -- one per output
// bit / per instance in the recovery examples -- are solved as lock-step gangs by one call; every
// element of the result is what m4ri_solve would return for that system.  `devices`: None (default) = the module's default
// device, "all" = every visible GPU, an int, or a sequence of device indices -- the systems are sharded in contiguous blocks over them,
// one host thread per entry inside the library (gf2bv_solve_batch_digits_multi), results in input order.
PyObject *py_m4ri_solve_many(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	if (nargs != 3 && nargs != 4) { PyErr_SetString(PyExc_TypeError, "m4ri_solve_many requires 3 arguments"); return nullptr; }
	std::vector<int> devs;
	if (!parse_devices(nargs == 4 ? args[3] : Py_None, &devs)) return nullptr;
	PyObject *systems = args[0];
	if (!PyList_Check(systems)) {
		PyErr_SetString(PyExc_TypeError, "The first argument must be a list of equation lists");
		return nullptr;
	}
	Py_ssize_t cols;
	long mode;
	if (!parse_cols_mode(args[1], args[2], &cols, &mode)) return nullptr;
	const Py_ssize_t nsys = PyList_GET_SIZE(systems);
	if (nsys == 0) return PyList_New(0);
	Py_ssize_t rows = -1;
	DigitGather dg;
	dg.hold = true;                        // later chunks are gathered after the GIL was dropped: own the ints for the whole call
	for (Py_ssize_t s = 0; s < nsys; s++) {
		PyObject *list = PyList_GET_ITEM(systems, s);
		if (!PyList_Check(list)) {
			PyErr_SetString(PyExc_TypeError, "The first argument must be a list of equation lists");
			return nullptr;
		}
		if (rows < 0) rows = PyList_GET_SIZE(list);
		if (PyList_GET_SIZE(list) != rows) {
			PyErr_SetString(PyExc_ValueError, "All systems of a batch need the same number of rows, pad with zeros.");
			return nullptr;
		}
		if (!rows_cover_cols(rows, cols)) return nullptr;
		if (!dg.add(list, cols)) return nullptr;
	}
	// The digits go to the library in CHUNKS of whole systems, at most GF2BV_BATCH_CHUNK_MB MiB each (default 2048; an even
	// number of systems per chunk, so that the library still forms two gangs of it): chunk k + 1 is gathered (GIL held, as for
	// one system) while chunk k is being solved by a thread of its own, and the two page-locked buffers the chunks alternate
	// between are recycled by the library's staging pool.  Gathering ALL the digits first -- 16 MT19937 recovery systems are
	// 800 MB, 64 systems of 32768^2 are 8.6 GB -- meant page-locking (or page-faulting) that much on every call: 226 of the
	// 270 ms of the 16-system call, where the solves take 44 (profiles/r05_mt_many.txt).
	const size_t total_digits = (size_t)dg.off.back();
	size_t chunk_bytes = (size_t)2048 << 20;
	if (const char *e = getenv("GF2BV_BATCH_CHUNK_MB")) { long v = atol(e); if (v >= 1) chunk_bytes = (size_t)v << 20; }
	Py_ssize_t chunk_sys = nsys;
	if (total_digits * sizeof(uint32_t) > chunk_bytes) {
		const size_t per_sys = std::max<size_t>(1, total_digits * sizeof(uint32_t) / (size_t)nsys);
		chunk_sys = (Py_ssize_t)std::max<size_t>(1, chunk_bytes / per_sys);
		if (chunk_sys >= 2) chunk_sys &= ~(Py_ssize_t)1;
		// equal chunks
		const Py_ssize_t nchunks = (nsys + chunk_sys - 1) / chunk_sys;
		chunk_sys = (nsys + nchunks - 1) / nchunks;
		if (chunk_sys >= 2 && (chunk_sys & 1) && chunk_sys < nsys) chunk_sys++;
	}
	std::vector<gf2bv_result *> res((size_t)nsys, nullptr);
	std::vector<int> sysdev((size_t)nsys, devs[0]);
	struct Chunk {
		Staging st;
		std::vector<int64_t> rel;                  // the chunk's offsets, from 0
		Py_ssize_t s0 = 0, s1 = 0;
		std::thread th;
		int rc = GF2BV_OK;
		std::string err;
		bool running = false;
		~Chunk() { if (th.joinable()) th.join(); }      // (never left running: an exception on the way out must not meet a live thread)
	} ck[2];
	int rc = GF2BV_OK;
	std::string err;
	auto join = [&](Chunk &c) {
		if (!c.running) return;
		Py_BEGIN_ALLOW_THREADS
		c.th.join();
		Py_END_ALLOW_THREADS
		c.running = false;
		c.st.drop();
		if (c.rc != GF2BV_OK && rc == GF2BV_OK) { rc = c.rc; err = c.err; }
	};
	bool pyerr = false;
	int which = 0;
	for (Py_ssize_t s0 = 0; s0 < nsys && rc == GF2BV_OK; s0 += chunk_sys, which ^= 1) {
		Chunk &c = ck[which];
		join(c);                                   // (the chunk before the previous one: its buffer is free again)
		if (rc != GF2BV_OK) break;
		c.s0 = s0; c.s1 = std::min<Py_ssize_t>(nsys, s0 + chunk_sys);
		const size_t r0 = (size_t)(c.s0 * rows), r1 = (size_t)(c.s1 * rows);
		if (!dg.gather_rows(r0, r1, chunk_bytes + chunk_bytes / 2, c.st)) { pyerr = true; break; }
		try { c.rel.assign(dg.off.begin() + (ptrdiff_t)r0, dg.off.begin() + (ptrdiff_t)r1 + 1); }
		catch (const std::bad_alloc &) { PyErr_NoMemory(); pyerr = true; break; }
		const int64_t base = c.rel[0];
		for (int64_t &o : c.rel) o -= base;
		// (the share -> device map of gf2bv_solve_batch_digits_multi: share k = systems floor(n k / shares) ..)
		const Py_ssize_t n = c.s1 - c.s0, nsh = std::min<Py_ssize_t>((Py_ssize_t)devs.size(), n);
		for (Py_ssize_t t = 0, share = 0; t < n; t++) {
			while (share + 1 < nsh && n * (share + 1) / nsh <= t) share++;
			sysdev[(size_t)(c.s0 + t)] = devs[(size_t)share];
		}
		join(ck[which ^ 1]);                       // one chunk on the device(s) at a time
		if (rc != GF2BV_OK) break;
		c.rc = GF2BV_OK; c.err.clear();
		c.running = true;
		try {
			c.th = std::thread([&c, &res, &devs, rows, cols, mode]() {
				c.rc = gf2bv_solve_batch_digits_multi(c.st.digits, c.rel.data(), PyLong_SHIFT, c.s1 - c.s0, rows, cols, (int)mode,
				                                      devs.data(), (int)devs.size(), res.data() + c.s0);
				if (c.rc != GF2BV_OK) c.err = gf2bv_last_error();      // (the message is per thread)
			});
		} catch (const std::system_error &) {
			c.running = false;
			rc = GF2BV_ERR_HIP; err = "could not start the solve thread";
		}
	}
	join(ck[0]); join(ck[1]);
	if (pyerr || rc != GF2BV_OK) {
		for (gf2bv_result *r : res) if (r) gf2bv_result_free(r);
		return pyerr ? nullptr : raise_rc(rc, "solve", err.c_str());
	}
	PyObject *out = PyList_New(nsys);
	Py_ssize_t done = 0;
	for (; out && done < nsys; done++) {
		PyObject *item = result_to_py(res[done], mode, sysdev[(size_t)done]);      // frees res[done]
		if (!item) { done++; Py_CLEAR(out); break; }
		PyList_SET_ITEM(out, done, item);
	}
	for (Py_ssize_t t = done; t < nsys; t++) gf2bv_result_free(res[t]);
	return out;
}

// to_bits(n, a): tuple of n bools, LSB first, zero-extended (_internal.c:504-531)
PyObject *py_to_bits(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	if (nargs != 2) { PyErr_SetString(PyExc_TypeError, "to_bits requires 2 arguments"); return nullptr; }
	Py_ssize_t n = PyLong_AsSsize_t(args[0]);
	if (n < 0) {
		if (n == -1 && PyErr_Occurred()) return nullptr;
		PyErr_SetString(PyExc_ValueError, "n must be non-negative");
		return nullptr;
	}
	if (!PyLong_Check(args[1])) { PyErr_SetString(PyExc_TypeError, "a must be an integer"); return nullptr; }
	PyLongObject *a = (PyLongObject *)args[1];
	PyObject *t = PyTuple_New(n);
	if (!t) return nullptr;
	for (Py_ssize_t i = 0; i < n; i++) {
		PyObject *b = long_bit(a, i) ? Py_True : Py_False;
		Py_INCREF(b);
		PyTuple_SET_ITEM(t, i, b);
	}
	return t;
}

// xor_tuple(a, b): element-wise a[i] ^ b[i] (_internal.c:606-639)
PyObject *py_xor_tuple(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	if (nargs != 2) { PyErr_SetString(PyExc_TypeError, "xor_tuple requires 2 arguments"); return nullptr; }
	PyObject *a = args[0], *b = args[1];
	if (!PyTuple_Check(a) || !PyTuple_Check(b)) {
		PyErr_SetString(PyExc_TypeError, "a and b must be tuples");
		return nullptr;
	}
	const Py_ssize_t n = PyTuple_GET_SIZE(a);
	if (n != PyTuple_GET_SIZE(b)) {
		PyErr_SetString(PyExc_ValueError, "The length of a and b is not equal");
		return nullptr;
	}
	PyObject *t = PyTuple_New(n);
	if (!t) return nullptr;
	for (Py_ssize_t i = 0; i < n; i++) {
		PyObject *x = PyNumber_Xor(PyTuple_GET_ITEM(a, i), PyTuple_GET_ITEM(b, i));
		if (!x) {
			Py_DECREF(t);
			PyErr_SetString(PyExc_TypeError, "Failed to compute xor, list items must be integers");
			return nullptr;
		}
		PyTuple_SET_ITEM(t, i, x);
	}
	return t;
}

// tuple_where(cond, a, b): np.where-like; OVERWRITES cond in place and returns it; a / b may be
// scalars (_internal.c:641-676)
PyObject *py_tuple_where(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	if (nargs != 3) { PyErr_SetString(PyExc_TypeError, "tuple_where requires 3 arguments"); return nullptr; }
	PyObject *cond = args[0], *a = args[1], *b = args[2];
	if (!PyTuple_Check(cond)) { PyErr_SetString(PyExc_TypeError, "cond must be a list"); return nullptr; }
	const bool at = PyTuple_Check(a), bt = PyTuple_Check(b);
	const Py_ssize_t n = PyTuple_GET_SIZE(cond);
	if (at && PyTuple_GET_SIZE(a) != n) {
		PyErr_SetString(PyExc_ValueError, "The length of a and cond is not equal");
		return nullptr;
	}
	if (bt && PyTuple_GET_SIZE(b) != n) {
		PyErr_SetString(PyExc_ValueError, "The length of b and cond is not equal");
		return nullptr;
	}
	for (Py_ssize_t i = 0; i < n; i++) {
		PyObject *c = PyTuple_GET_ITEM(cond, i);
		int truth = PyObject_IsTrue(c);
		if (truth < 0) return nullptr;
		PyObject *pick = truth ? (at ? PyTuple_GET_ITEM(a, i) : a) : (bt ? PyTuple_GET_ITEM(b, i) : b);
		Py_INCREF(pick);
		PyTuple_SET_ITEM(cond, i, pick);
		Py_DECREF(c);
	}
	Py_INCREF(cond);
	return cond;
}

// mul_bit_quad(n, a, b, v, basis): OR basis[1+n+i(i-1)/2+j] into v for every j<i with
// a_i b_j ^ a_j b_i = 1 (_internal.c:538-604).  Caller-side helper of QuadraticSystem.
PyObject *py_mul_bit_quad(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	if (nargs != 5) { PyErr_SetString(PyExc_TypeError, "mul_bit_quad requires 5 arguments"); return nullptr; }
	Py_ssize_t n = PyLong_AsSsize_t(args[0]);
	if (n <= 0) {
		if (n == -1 && PyErr_Occurred()) return nullptr;
		PyErr_SetString(PyExc_ValueError, "n must be positive");
		return nullptr;
	}
	if (!PyLong_Check(args[1]) || !PyLong_Check(args[2]) || !PyLong_Check(args[3])) {
		PyErr_SetString(PyExc_TypeError, "a and b and v must be integers");
		return nullptr;
	}
	PyObject *basis = args[4];
	if (!PyList_Check(basis)) { PyErr_SetString(PyExc_TypeError, "basis must be a list"); return nullptr; }
	if (PyList_GET_SIZE(basis) != 1 + n + n * (n - 1) / 2) {
		PyErr_SetString(PyExc_ValueError, "The length of basis is not correct");
		return nullptr;
	}
	PyLongObject *a = (PyLongObject *)args[1], *b = (PyLongObject *)args[2];
	std::vector<char> ab((size_t)n), bb((size_t)n);
	for (Py_ssize_t i = 0; i < n; i++) { ab[i] = long_bit(a, i); bb[i] = long_bit(b, i); }
	PyObject *v = args[3];
	Py_INCREF(v);
	Py_ssize_t mi = 1 + n;
	for (Py_ssize_t i = 0; i < n; i++)
		for (Py_ssize_t j = 0; j < i; j++, mi++)
			if ((ab[i] & bb[j]) ^ (ab[j] & bb[i])) {
				PyObject *nv = PyNumber_Or(v, PyList_GET_ITEM(basis, mi));
				Py_DECREF(v);
				if (!nv) {
					PyErr_SetString(PyExc_TypeError, "Failed to compute or, list items must be integers");
					return nullptr;
				}
				v = nv;
			}
	return v;
}

// eqs_to_sage_mat_helper(eqs, cols) -> (png_bytes, affine_list)      (_internal.c:678-765)
// The reference renders the coefficient matrix as an image -- pixel (x = column, y = row) BLACK where the bit is set -- through
// libgd (dlopen at first use) and returns gdImagePngPtrEx(im, &size, 0): a palette PNG with colour 0 = black, 1 = white,
// compression level 0, which Sage's unpickle_matrix_mod2_dense_v2 reads back as entry = 1 - palette index.  Here the PNG is
// written directly (no libgd, no libpng, no zlib): signature, IHDR (bit depth 1, colour type 3 -- what libgd's writer picks
// for a two-colour palette), PLTE {000000, FFFFFF}, the scanlines (filter byte 0, pixels MSB first, padding bits white) as
// STORED deflate blocks (level 0) in IDAT chunks of at most 1 MiB, IEND.  Same pixels and palette as the reference's image;
// byte-for-byte equality with a particular libgd/libpng build is not claimed (chunking and zlib framing are the encoder's).
// affine[i] = bit 0 of eqs[i] as a bool; the reference leaves a NULL slot for an equation that is the int 0 (its bit loop
// never runs, _internal.c:741-752) -- get_eqs never passes one -- here that entry is False.
namespace png {
uint32_t crc_table[256];
bool crc_ready = false;
uint32_t crc32(uint32_t c, const unsigned char *p, size_t n)
{
	if (!crc_ready) {
		for (uint32_t i = 0; i < 256; i++) {
			uint32_t v = i;
			for (int k = 0; k < 8; k++) v = (v & 1) ? 0xEDB88320u ^ (v >> 1) : v >> 1;
			crc_table[i] = v;
		}
		crc_ready = true;
	}
	c = ~c;
	for (size_t i = 0; i < n; i++) c = crc_table[(c ^ p[i]) & 0xff] ^ (c >> 8);
	return ~c;
}
void be32(std::vector<unsigned char> &o, uint32_t v) { for (int s = 24; s >= 0; s -= 8) o.push_back((unsigned char)(v >> s)); }
void chunk(std::vector<unsigned char> &o, const char *type, const unsigned char *data, size_t n)
{
	be32(o, (uint32_t)n);
	const size_t at = o.size();
	o.insert(o.end(), type, type + 4);
	o.insert(o.end(), data, data + n);
	be32(o, crc32(0, o.data() + at, n + 4));
}
}  // namespace png

PyObject *py_sage_helper(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	if (nargs != 2) { PyErr_SetString(PyExc_TypeError, "eqs_to_sage_mat_helper requires 2 arguments"); return nullptr; }
	PyObject *list = args[0];
	if (!PyList_Check(list)) { PyErr_SetString(PyExc_TypeError, "The first argument equations must be a list"); return nullptr; }
	const Py_ssize_t cols = PyLong_AsSsize_t(args[1]);
	if (cols <= 0) {
		if (cols == -1 && PyErr_Occurred()) return nullptr;
		PyErr_SetString(PyExc_ValueError, "Number of columns must be positive");
		return nullptr;
	}
	const Py_ssize_t rows = PyList_GET_SIZE(list);
	if (cols > 0x7fffffff || rows > 0x7fffffff) { PyErr_SetString(PyExc_ValueError, "image dimensions exceed PNG's 2^31 - 1"); return nullptr; }
	for (Py_ssize_t i = 0; i < rows; i++)
		if (!PyLong_Check(PyList_GET_ITEM(list, i))) { PyErr_SetString(PyExc_TypeError, "All elements in the equations list must be integers"); return nullptr; }
	PyObject *affine = PyList_New(rows);
	if (!affine) return nullptr;
	try {
		const size_t rb = (size_t)(cols + 7) / 8, line = rb + 1;
		const size_t words = (size_t)(cols + 63) / 64;
		// the raw image (filter byte + packed pixels per row)
		std::vector<unsigned char> raw(line * (size_t)rows);
		std::vector<uint64_t> bits(words + 1);
		static unsigned char rev[256];
		static bool rev_ready = false;
		if (!rev_ready) { for (int v = 0; v < 256; v++) { int r = 0; for (int k = 0; k < 8; k++) if (v >> k & 1) r |= 0x80 >> k; rev[v] = (unsigned char)r; } rev_ready = true; }
		for (Py_ssize_t i = 0; i < rows; i++) {
			PyLongObject *v = (PyLongObject *)PyList_GET_ITEM(list, i);
			const Py_ssize_t nd = GF2_DIGIT_COUNT(v);
			PyObject *aff = (nd > 0 && (GF2_DIGITS(v)[0] & 1)) ? Py_True : Py_False;
			Py_INCREF(aff);
			PyList_SET_ITEM(affine, i, aff);
			// bits[c] = bit c + 1 of |v| for c < cols (the sign is ignored, bits above cols are ignored: _internal.c:41-59)
			std::fill(bits.begin(), bits.end(), 0);
			for (Py_ssize_t d = 0; d < nd; d++) {
				uint64_t val = GF2_DIGITS(v)[d];
				Py_ssize_t at = d * PyLong_SHIFT - 1;
				if (d == 0) { val >>= 1; at = 0; }
				if (at >= cols) break;
				bits[(size_t)at >> 6] |= val << (at & 63);
				if ((at & 63) + PyLong_SHIFT > 64) bits[((size_t)at >> 6) + 1] |= val >> (64 - (at & 63));
			}
			if (cols & 63) bits[words - 1] &= (~0ull >> (64 - (cols & 63)));
			unsigned char *dst = raw.data() + line * (size_t)i;
			dst[0] = 0;                                       // filter type None
			for (size_t k = 0; k < rb; k++) dst[1 + k] = rev[(unsigned char)~(bits[k >> 3] >> (8 * (k & 7)))];      // set bit -> index 0 (black)
		}
		// zlib stream of stored blocks
		std::vector<unsigned char> z;
		z.reserve(raw.size() + raw.size() / 65535 * 5 + 16);
		z.push_back(0x78); z.push_back(0x01);
		uint32_t a1 = 1, a2 = 0;
		size_t pos = 0;
		do {
			const size_t n = std::min<size_t>(65535, raw.size() - pos);
			z.push_back(pos + n == raw.size() ? 1 : 0);
			z.push_back((unsigned char)(n & 0xff)); z.push_back((unsigned char)(n >> 8));
			z.push_back((unsigned char)(~n & 0xff)); z.push_back((unsigned char)((~n >> 8) & 0xff));
			z.insert(z.end(), raw.begin() + pos, raw.begin() + pos + n);
			for (size_t k = 0; k < n;) {                      // adler32, reduced every 5552 bytes
				const size_t m = std::min<size_t>(5552, n - k);
				for (size_t e = 0; e < m; e++) { a1 += raw[pos + k + e]; a2 += a1; }
				a1 %= 65521; a2 %= 65521; k += m;
			}
			pos += n;
		} while (pos < raw.size());
		png::be32(z, (a2 << 16) | a1);
		std::vector<unsigned char>().swap(raw);
		std::vector<unsigned char> out;
		out.reserve(z.size() + z.size() / (1 << 20) * 12 + 128);
		static const unsigned char sig[8] = { 0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a };
		out.insert(out.end(), sig, sig + 8);
		std::vector<unsigned char> ihdr;
		png::be32(ihdr, (uint32_t)cols); png::be32(ihdr, (uint32_t)rows);
		ihdr.push_back(1); ihdr.push_back(3); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);
		png::chunk(out, "IHDR", ihdr.data(), ihdr.size());
		static const unsigned char plte[6] = { 0, 0, 0, 255, 255, 255 };
		png::chunk(out, "PLTE", plte, 6);
		for (size_t at = 0; at < z.size(); at += (size_t)1 << 20)
			png::chunk(out, "IDAT", z.data() + at, std::min<size_t>((size_t)1 << 20, z.size() - at));
		png::chunk(out, "IEND", nullptr, 0);
		PyObject *bytes = PyBytes_FromStringAndSize((const char *)out.data(), (Py_ssize_t)out.size());
		if (!bytes) { Py_DECREF(affine); return nullptr; }
		PyObject *ret = PyTuple_Pack(2, bytes, affine);
		Py_DECREF(bytes); Py_DECREF(affine);
		return ret;
	} catch (const std::bad_alloc &) {
		Py_DECREF(affine);
		return PyErr_NoMemory();
	}
}

// AffineSpace.quad_search(n_lin, max_enum=32, max_solutions=65536, first=False): the consistent points of the space (every
// product coordinate the product of its linear bits), in iteration order, found on the device (gf2bv_quad_search_alloc).
// More than max_solutions points: ValueError -- or, with first=True, the first max_solutions of them.  Not in the reference.
// AffineSpace.cubic_search, AffineSpace.quartic_search: the same over the degree-3 and the degree-4 columns (gf2bv_cubic_search_alloc,
// gf2bv_quartic_search_alloc), CubicSearchGaveUp / QuarticSearchGaveUp when it gives up.
PyObject *space_search(AffineSpaceObject *self, PyObject *const *args, Py_ssize_t nargs, int degree)
{
	const bool cubic = degree >= 3;               // (the texts the degrees above 2 share)
	const auto entry = degree == 4 ? gf2bv_quartic_search_alloc : degree == 3 ? gf2bv_cubic_search_alloc : gf2bv_quad_search_alloc;
	const char *name = degree == 4 ? "quartic_search" : degree == 3 ? "cubic_search" : "quad_search";
	if (nargs < 1 || nargs > 4) {
		PyErr_Format(PyExc_TypeError, "%s(n_lin, max_enum=32, max_solutions=65536, first=False)", name);
		return nullptr;
	}
	const long long n_lin = PyLong_AsLongLong(args[0]);
	const long long max_enum = nargs > 1 ? PyLong_AsLongLong(args[1]) : 32;
	const long long max_sol = nargs > 2 ? PyLong_AsLongLong(args[2]) : 65536;
	if (PyErr_Occurred()) return nullptr;
	const int first = nargs > 3 ? PyObject_IsTrue(args[3]) : 0;
	if (first < 0) return nullptr;
	if (max_enum < 0 || max_enum > 40) { PyErr_SetString(PyExc_ValueError, "max_enum must be 0..40"); return nullptr; }
	if (max_sol < 0) { PyErr_SetString(PyExc_ValueError, "max_solutions must be >= 0"); return nullptr; }
	const int device = self->device >= 0 ? self->device : default_device();
	int64_t count = 0, lin_rank = 0;
	uint64_t *pts = nullptr;                  // exactly min(count, max_solutions) points, owned by the library
	int rc;
	Py_BEGIN_ALLOW_THREADS
	rc = entry(self->origin, self->basis, self->dim, self->words, n_lin, (int)max_enum, max_sol, device, &count, &lin_rank, &pts);
	Py_END_ALLOW_THREADS
	if (rc == GF2BV_ERR_NOMEM && count > max_sol) {     // more than 2^22 points: too many to order
		gf2bv_quad_free(pts);
		if (first)
			PyErr_Format(PyExc_ValueError, "%lld consistent points: too many to order (at most 4194304); add equations to narrow "
			             "the system", (long long)count);
		else
			PyErr_Format(PyExc_ValueError, "%lld consistent points, more than max_solutions (%lld)", (long long)count, max_sol);
		return nullptr;
	}
	if (rc != GF2BV_OK) { gf2bv_quad_free(pts); return raise_rc(rc, name); }
	if (count < 0) {
		gf2bv_quad_free(pts);
		PyObject *msg = PyUnicode_FromFormat(cubic ? "the search gave up: the space's projection onto the %lld linear coordinates has rank %lld, "
		                                             "and the affine elimination does not get it down to max_enum (%lld) or it is above 64"
		                                           : "the search gave up: the space's projection onto the %lld linear coordinates has rank %lld, "
		                                             "and neither a search (max_enum %lld) nor relinearisation gets below it",
		                                     n_lin, (long long)lin_rank, max_enum);
		if (msg) {
			PyObject *e = Py_BuildValue("(NL)", msg, (long long)lin_rank);
			if (e) { PyErr_SetObject(degree == 4 ? QuarticGaveUp : degree == 3 ? CubicGaveUp : QuadGaveUp, e); Py_DECREF(e); }
		}
		return nullptr;
	}
	if (count > max_sol && !first) {
		gf2bv_quad_free(pts);
		PyErr_Format(PyExc_ValueError, "%lld consistent points, more than max_solutions (%lld)", (long long)count, max_sol);
		return nullptr;
	}
	const int64_t n = std::min<int64_t>(count, max_sol);
	PyObject *t = PyTuple_New((Py_ssize_t)n);
	for (int64_t k = 0; t && k < n; k++) {
		PyObject *v = words_to_pylong(pts + k * self->words, self->words);
		if (!v) { Py_CLEAR(t); break; }
		PyTuple_SET_ITEM(t, k, v);
	}
	gf2bv_quad_free(pts);
	return t;
}

PyObject *space_quad_search(AffineSpaceObject *self, PyObject *const *args, Py_ssize_t nargs) { return space_search(self, args, nargs, 2); }
PyObject *space_cubic_search(AffineSpaceObject *self, PyObject *const *args, Py_ssize_t nargs) { return space_search(self, args, nargs, 3); }
PyObject *space_quartic_search(AffineSpaceObject *self, PyObject *const *args, Py_ssize_t nargs) { return space_search(self, args, nargs, 4); }

// _space_from_ints(cols, origin, basis): build an AffineSpace from host integers.  Not part of the
// reference surface; lets the CPU test-suite exercise get()/iteration order without a GPU.
PyObject *py_space_from_ints(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	if (nargs != 3 || !PyLong_Check(args[1]) || !PyTuple_Check(args[2])) {
		PyErr_SetString(PyExc_TypeError, "_space_from_ints(cols, origin, basis_tuple)");
		return nullptr;
	}
	Py_ssize_t cols = PyLong_AsSsize_t(args[0]);
	if (cols <= 0) { if (!PyErr_Occurred()) PyErr_SetString(PyExc_ValueError, "cols must be positive"); return nullptr; }
	const int64_t words = (cols + 63) / 64;
	const int64_t dim = PyTuple_GET_SIZE(args[2]);
	AffineSpaceObject *sp = (AffineSpaceObject *)AffineSpace_Type->tp_alloc(AffineSpace_Type, 0);
	if (!sp) return nullptr;
	sp->dim = dim;
	sp->words = words;
	sp->device = -1;                 // host-built: walked on the host (no GPU needed for the host-logic tests)
	sp->origin = (uint64_t *)calloc((size_t)words, sizeof(uint64_t));
	sp->basis = (uint64_t *)calloc((size_t)((dim * words) > 0 ? dim * words : 1), sizeof(uint64_t));
	if (!sp->origin || !sp->basis) { Py_DECREF(sp); return PyErr_NoMemory(); }
	for (int64_t k = -1; k < dim; k++) {
		PyObject *v = k < 0 ? args[1] : PyTuple_GET_ITEM(args[2], k);
		if (!PyLong_Check(v)) { Py_DECREF(sp); PyErr_SetString(PyExc_TypeError, "integers expected"); return nullptr; }
		uint64_t *dst = k < 0 ? sp->origin : sp->basis + k * words;
		for (Py_ssize_t i = 0; i < cols; i++)
			if (long_bit((PyLongObject *)v, i)) dst[i >> 6] |= (uint64_t)1 << (i & 63);
	}
	return (PyObject *)sp;
}

// m4ri_compose_packed(a, ra, n, b, nb[, device]) -> bytearray: the forms `a` (ra x ceil((n + 1) / 64) 64-bit words, m4ri_solve_packed's
// bit order) with the images `b` (n x ceil((nb + 1) / 64) words: row g replaces unknown g) substituted on the device
// (gf2bv_compose_words); the result is ra x ceil((nb + 1) / 64) words.  New entry, no counterpart in the reference.
// m4ri_power_packed(b, n, k[, device]) -> bytearray: the self-map `b` (n x ceil((n + 1) / 64) words) substituted into itself k times by
// square-and-multiply on the device (gf2bv_compose_power_words); k a buffer of little-endian 64-bit words, at least one.
bool packed_forms(HeldBuffer &hb, PyObject *buf, Py_ssize_t rows, Py_ssize_t unknowns, const char *what)
{
	if (!hb.take(buf, PyBUF_C_CONTIGUOUS)) return false;
	if (rows < 0 || unknowns < 1 || unknowns >= PY_SSIZE_T_MAX / 16 || hb.view.len != rows * ((unknowns + 64) / 64) * 8) {
		PyErr_Format(PyExc_ValueError, "%s must hold rows x ceil((unknowns + 1) / 64) 64-bit words", what);
		return false;
	}
	return true;
}

template <class F>
PyObject *composed_rows(const char *what, Py_ssize_t rows, Py_ssize_t words, F &&call)
{
	PyObject *out = PyByteArray_FromStringAndSize(nullptr, rows * words * 8);
	if (!out) return nullptr;
	uint64_t *dst = reinterpret_cast<uint64_t *>(PyByteArray_AS_STRING(out));
	int rc;
	std::string msg;
	Py_BEGIN_ALLOW_THREADS
	rc = call(dst);
	if (rc) msg = gf2bv_last_error();
	Py_END_ALLOW_THREADS
	if (rc) { Py_DECREF(out); return raise_rc(rc, what, msg.c_str()); }
	return out;
}

PyObject *py_m4ri_compose_packed(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_compose_packed", 5, args, nargs, &device)) return nullptr;
	const Py_ssize_t ra = PyLong_AsSsize_t(args[1]), n = PyLong_AsSsize_t(args[2]), nb = PyLong_AsSsize_t(args[4]);
	if (PyErr_Occurred()) return nullptr;
	HeldBuffer a, b;
	if (!packed_forms(a, args[0], ra, n, "a") || !packed_forms(b, args[3], n, nb, "b")) return nullptr;
	const Py_ssize_t wa = (n + 64) / 64, wb = (nb + 64) / 64;
	static const uint64_t none = 0;               // (no rows: the library still wants a pointer)
	return composed_rows("composition", ra, wb, [&](uint64_t *dst) {
		return gf2bv_compose_words(ra ? static_cast<const uint64_t *>(a.view.buf) : &none, ra, wa, n, static_cast<const uint64_t *>(b.view.buf), wb, nb,
		                           ra ? dst : const_cast<uint64_t *>(&none), wb, device);
	});
}

PyObject *py_m4ri_power_packed(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_power_packed", 3, args, nargs, &device)) return nullptr;
	const Py_ssize_t n = PyLong_AsSsize_t(args[1]);
	if (PyErr_Occurred()) return nullptr;
	HeldBuffer b, k;
	if (!packed_forms(b, args[0], n, n, "b") || !k.take(args[2], PyBUF_C_CONTIGUOUS)) return nullptr;
	if (k.view.len < 8 || k.view.len % 8) { PyErr_SetString(PyExc_ValueError, "k must hold at least one 64-bit word"); return nullptr; }
	const Py_ssize_t w = (n + 64) / 64;
	return composed_rows("power", n, w, [&](uint64_t *dst) {
		return gf2bv_compose_power_words(static_cast<const uint64_t *>(b.view.buf), w, n, static_cast<const uint64_t *>(k.view.buf), k.view.len / 8, dst, w, device);
	});
}

// m4ri_unroll_packed(a, ra, n, b, start_words, step_words, count[, device]) -> bytearray: the forms `a` (ra x ceil((n + 1) / 64) words)
// watched while the self-map `b` steps -- count x ra rows, time-major, row i x ra + r = a[r] with b substituted start + i x step times
// (gf2bv_compose_unroll_words); start and step are buffers of little-endian 64-bit words, at least one each.
PyObject *py_m4ri_unroll_packed(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
	int device;
	if (!entry_device("m4ri_unroll_packed", 7, args, nargs, &device)) return nullptr;
	const Py_ssize_t ra = PyLong_AsSsize_t(args[1]), n = PyLong_AsSsize_t(args[2]), count = PyLong_AsSsize_t(args[6]);
	if (PyErr_Occurred()) return nullptr;
	HeldBuffer a, b, start, step;
	if (!packed_forms(a, args[0], ra, n, "a") || !packed_forms(b, args[3], n, n, "b")) return nullptr;
	if (!start.take(args[4], PyBUF_C_CONTIGUOUS) || !step.take(args[5], PyBUF_C_CONTIGUOUS)) return nullptr;
	if (start.view.len < 8 || start.view.len % 8 || step.view.len < 8 || step.view.len % 8) {
		PyErr_SetString(PyExc_ValueError, "start and step must hold at least one 64-bit word each");
		return nullptr;
	}
	const Py_ssize_t w = (n + 64) / 64;
	if (count < 0 || (ra > 0 && count > PY_SSIZE_T_MAX / 8 / w / ra)) { PyErr_SetString(PyExc_ValueError, "count must not be negative, and count x ra rows must fit in memory"); return nullptr; }
	static const uint64_t none = 0;               // (no rows: the library still wants a pointer)
	const bool empty = ra == 0 || count == 0;
	return composed_rows("unrolling", count * ra, w, [&](uint64_t *dst) {
		return gf2bv_compose_unroll_words(ra ? static_cast<const uint64_t *>(a.view.buf) : &none, ra, w, n, static_cast<const uint64_t *>(b.view.buf), w,
		                                  static_cast<const uint64_t *>(start.view.buf), start.view.len / 8,
		                                  static_cast<const uint64_t *>(step.view.buf), step.view.len / 8, count,
		                                  empty ? const_cast<uint64_t *>(&none) : dst, w, device);
	});
}

PyObject *py_device_count(PyObject *, PyObject *) { return PyLong_FromLong(gf2bv_device_count()); }
PyObject *py_get_default_device(PyObject *, PyObject *) { return PyLong_FromLong(default_device()); }
PyObject *py_set_default_device(PyObject *, PyObject *arg)
{
	int d;
	if (arg == Py_None) { PyErr_SetString(PyExc_TypeError, "device must be an int"); return nullptr; }
	if (!parse_device(arg, &d)) return nullptr;
	g_default_device = d;
	Py_RETURN_NONE;
}

// content ids of the two binaries (gf2bv_amd/build.py compiles them in; the marker lets build.py read the shim's without loading it)
#ifndef GF2BV_SHIM_ID
#define GF2BV_SHIM_ID "unknown"
#endif
const char g_shim_id[] = "GF2BV_SHIM_ID=" GF2BV_SHIM_ID;
PyObject *py_build_id(PyObject *, PyObject *) { return Py_BuildValue("{s:s,s:s}", "hip", gf2bv_build_id(), "shim", g_shim_id + 14); }

#define FAST(fn) (PyCFunction)(void (*)(void))(fn)
PyMethodDef module_methods[] = {
	{"m4ri_solve", FAST(py_m4ri_solve), METH_FASTCALL,
	 "m4ri_solve(equations, cols, mode, device=None)\n--\n\nSolve the linear system on the MI355X; None when inconsistent."},
	{"m4ri_solve_packed", FAST(py_m4ri_solve_packed), METH_FASTCALL,
	 "m4ri_solve_packed(buffer, rows, words, cols, mode, device=None)\n--\n\nm4ri_solve on equations already packed as rows x words 64-bit words (equation-int bit order)."},
	{"m4ri_compose_packed", FAST(py_m4ri_compose_packed), METH_FASTCALL,
	 "m4ri_compose_packed(a, ra, n, b, nb, device=None)\n--\n\nThe packed forms a (ra rows over n unknowns) with the packed images b (n rows over nb unknowns) substituted on the GPU: a bytearray of ra x ceil((nb + 1) / 64) 64-bit words."},
	{"m4ri_power_packed", FAST(py_m4ri_power_packed), METH_FASTCALL,
	 "m4ri_power_packed(b, n, k, device=None)\n--\n\nThe packed self-map b (n rows over n unknowns) substituted into itself k times (k: little-endian 64-bit words) by square-and-multiply on the GPU: a bytearray of n x ceil((n + 1) / 64) words."},
	{"m4ri_unroll_packed", FAST(py_m4ri_unroll_packed), METH_FASTCALL,
	 "m4ri_unroll_packed(a, ra, n, b, start_words, step_words, count, device=None)\n--\n\nThe packed forms a (ra rows over n unknowns) watched while the packed self-map b steps on the GPU: a bytearray of count x ra x ceil((n + 1) / 64) words, time-major -- row i x ra + r is a[r] with b substituted start + i x step times (start, step: little-endian 64-bit words)."},
	{"m4ri_solve_quad_packed", FAST(py_m4ri_solve_quad_packed), METH_FASTCALL,
	 "m4ri_solve_quad_packed(lin, term_off, ta, tb, n_lin, rows, mode, device=None)\n--\n\nm4ri_solve on a quadratic system kept factored (linear forms and products of two linear forms, packed 64-bit words): expanded into the linearised matrix on the GPU."},
	{"m4ri_solve_xl3", FAST(py_m4ri_solve_xl<3>), METH_FASTCALL,
	 "m4ri_solve_xl3(equations, n_lin, mode, device=None)\n--\n\nDegree-3 XL: QuadraticSystem equation ints multiplied by 1 and by every unknown on the GPU and solved over the monomials of degree <= 3."},
	{"m4ri_solve_quartic_packed", FAST(py_m4ri_solve_quartic_packed), METH_FASTCALL,
	 "m4ri_solve_quartic_packed(lin, off2, ta, tb, off3, ua, ub, uc, off4, va, vb, vc, vd, n_lin, rows, mode, device=None)\n--\n\nm4ri_solve on a quartic system kept factored (a linear form, products of two, of three and of four affine forms, packed 64-bit words; exact products): expanded over the monomials of degree <= 4 on the GPU."},
	{"m4ri_solve_cubic_packed", FAST(py_m4ri_solve_cubic_packed), METH_FASTCALL,
	 "m4ri_solve_cubic_packed(lin, off2, ta, tb, off3, ua, ub, uc, n_lin, rows, mode, device=None)\n--\n\nm4ri_solve on a cubic system kept factored (a linear form, products of two and of three affine forms, packed 64-bit words; exact products): expanded over the monomials of degree <= 3 on the GPU."},
	{"m4ri_solve_xl3_quad_packed", FAST(py_m4ri_solve_xl_quad_packed<3>), METH_FASTCALL,
	 "m4ri_solve_xl3_quad_packed(lin, term_off, ta, tb, n_lin, mode, device=None)\n--\n\nm4ri_solve_xl3 on a quadratic system kept factored: expanded, multiplied and solved on the GPU."},
	{"m4ri_solve_xl3_guess", FAST(py_m4ri_solve_xl_guess<3>), METH_FASTCALL,
	 "m4ri_solve_xl3_guess(equations, n_lin, guess, a0, na, mode, device=None)\n--\n\nHybrid XL: the guessed unknowns substituted for the assignments a0 .. a0 + na - 1 and every assignment's degree-3 XL system solved on the GPU as one batch."},
	{"m4ri_solve_xl3_guess_quad_packed", FAST(py_m4ri_solve_xl_guess_quad_packed<3>), METH_FASTCALL,
	 "m4ri_solve_xl3_guess_quad_packed(lin, term_off, ta, tb, n_lin, guess, a0, na, mode, device=None)\n--\n\nm4ri_solve_xl3_guess on a quadratic system kept factored."},
	{"m4ri_solve_xl4_cubic_packed", FAST(py_m4ri_solve_xl4_cubic_packed), METH_FASTCALL,
	 "m4ri_solve_xl4_cubic_packed(lin, off2, ta, tb, off3, ua, ub, uc, n_lin, mode, device=None)\n--\n\nDegree-4 XL on a cubic system kept factored: every equation multiplied by 1 and by each unknown on the GPU, solved over the monomials of degree <= 4."},
	{"m4ri_solve_xl4", FAST(py_m4ri_solve_xl<4>), METH_FASTCALL,
	 "m4ri_solve_xl4(equations, n_lin, mode, device=None)\n--\n\nDegree-4 XL: m4ri_solve_xl3 with the products by every pair of unknowns too, solved over the monomials of degree <= 4."},
	{"m4ri_solve_xl4_quad_packed", FAST(py_m4ri_solve_xl_quad_packed<4>), METH_FASTCALL,
	 "m4ri_solve_xl4_quad_packed(lin, term_off, ta, tb, n_lin, mode, device=None)\n--\n\nm4ri_solve_xl4 on a quadratic system kept factored."},
	{"m4ri_solve_xl4_guess_cubic_packed", FAST(py_m4ri_solve_xl4_guess_cubic_packed), METH_FASTCALL,
	 "m4ri_solve_xl4_guess_cubic_packed(lin, off2, ta, tb, off3, ua, ub, uc, n_lin, guess, a0, na, mode, device=None)\n--\n\nHybrid degree-4 XL on a cubic system kept factored: the guessed unknowns substituted for the assignments a0 .. a0 + na - 1 and every assignment's system solved on the GPU as one batch."},
	{"m4ri_solve_xl4_guess", FAST(py_m4ri_solve_xl_guess<4>), METH_FASTCALL,
	 "m4ri_solve_xl4_guess(equations, n_lin, guess, a0, na, mode, device=None)\n--\n\nHybrid XL at degree 4: m4ri_solve_xl3_guess with every assignment's degree-4 XL system."},
	{"m4ri_solve_xl4_guess_quad_packed", FAST(py_m4ri_solve_xl_guess_quad_packed<4>), METH_FASTCALL,
	 "m4ri_solve_xl4_guess_quad_packed(lin, term_off, ta, tb, n_lin, guess, a0, na, mode, device=None)\n--\n\nm4ri_solve_xl4_guess on a quadratic system kept factored."},
	{"m4ri_solve_rhs", FAST(py_m4ri_solve_rhs), METH_FASTCALL,
	 "m4ri_solve_rhs(equations, cols, mode, rhs, device=None)\n--\n\nSolve one coefficient matrix against every right-hand side in rhs (bit r = affine term of equation r) with one elimination; list of m4ri_solve results."},
	{"m4ri_factor", FAST(py_m4ri_factor), METH_FASTCALL,
	 "m4ri_factor(equations, cols, mode, device=None)\n--\n\nFactor the coefficient matrix once (bit 0 of every equation ignored); Factorization.solve(rhs) equals m4ri_solve_rhs(equations, cols, mode, rhs)."},
	{"m4ri_factor_packed", FAST(py_m4ri_factor_packed), METH_FASTCALL,
	 "m4ri_factor_packed(buffer, rows, words, cols, mode, device=None)\n--\n\nm4ri_factor on m4ri_solve_packed's buffer."},
	{"m4ri_factor_quad_packed", FAST(py_m4ri_factor_quad_packed), METH_FASTCALL,
	 "m4ri_factor_quad_packed(lin, term_off, ta, tb, n_lin, rows, mode, device=None)\n--\n\nA Factorization of the linearised matrix of factored quadratic equations, expanded on the device."},
	{"m4ri_solve_rhs_packed", FAST(py_m4ri_solve_rhs_packed), METH_FASTCALL,
	 "m4ri_solve_rhs_packed(buffer, rows, words, cols, mode, rhs, device=None)\n--\n\nm4ri_solve_rhs on m4ri_solve_packed's buffer; rhs a list of ints or an nrhs x words uint64 array."},
	{"m4ri_solve_rhs_quad_packed", FAST(py_m4ri_solve_rhs_quad_packed), METH_FASTCALL,
	 "m4ri_solve_rhs_quad_packed(lin, term_off, ta, tb, n_lin, rows, mode, rhs, device=None)\n--\n\nm4ri_solve_rhs on factored quadratic equations, expanded on the device."},
	{"m4ri_solve_many_quad_packed", FAST(py_m4ri_solve_many_quad_packed), METH_FASTCALL,
	 "m4ri_solve_many_quad_packed(lin, term_off, ta, tb, sys_row_off, n_lin, rows, mode, device=None)\n--\n\nIndependent factored quadratic systems of one concatenated term set, expanded by one launch and solved as lock-step gangs."},
	{"m4ri_solve_many", FAST(py_m4ri_solve_many), METH_FASTCALL,
	 "m4ri_solve_many(systems, cols, mode, devices=None)\n--\n\nSolve a list of same-shape systems in one batched call, sharded over the given GPUs (None: the default device, \"all\": every visible one); list of m4ri_solve results."},
	{"to_bits", FAST(py_to_bits), METH_FASTCALL, "to_bits(n, a)\n--\n\nLow n bits of a, LSB first."},
	{"mul_bit_quad", FAST(py_mul_bit_quad), METH_FASTCALL, "mul_bit_quad(n, a, b, v, basis)\n--\n\n"},
	{"xor_tuple", FAST(py_xor_tuple), METH_FASTCALL, "xor_tuple(a, b)\n--\n\nElement-wise xor."},
	{"tuple_where", FAST(py_tuple_where), METH_FASTCALL, "tuple_where(cond, a, b)\n--\n\nIn-place select."},
	{"eqs_to_sage_mat_helper", FAST(py_sage_helper), METH_FASTCALL,
	 "eqs_to_sage_mat_helper(equations, cols)\n--\n\n(png_bytes, affine): the coefficient matrix as a two-colour PNG (black = 1) for Sage's unpickle_matrix_mod2_dense_v2, and the affine bits."},
	{"_space_from_ints", FAST(py_space_from_ints), METH_FASTCALL, "test hook: AffineSpace from ints"},
	{"device_count", py_device_count, METH_NOARGS, "number of visible HIP devices"},
	{"build_id", py_build_id, METH_NOARGS, "content hashes of the sources libgf2bv_hip.so and this module were compiled from"},
	{"get_default_device", py_get_default_device, METH_NOARGS, "the device solves run on when no `device` argument is given"},
	{"set_default_device", py_set_default_device, METH_O, "set_default_device(d)\n--\n\nselect the GPU for solves without a `device` argument"},
	{nullptr, nullptr, 0, nullptr}};

PyModuleDef module_def = {PyModuleDef_HEAD_INIT, "_internal", "gf2bv_amd native boundary (HIP solver)", -1,
                          module_methods, nullptr, nullptr, nullptr, nullptr};

}  // namespace

PyMODINIT_FUNC PyInit__internal(void)
{
	PyObject *m = PyModule_Create(&module_def);
	if (!m) return nullptr;
	AffineSpace_Type = (PyTypeObject *)PyType_FromSpec(&space_spec);
	SpaceIterGray_Type = (PyTypeObject *)PyType_FromSpec(&gray_spec);
	SpaceIterSlow_Type = (PyTypeObject *)PyType_FromSpec(&slow_spec);
	Factorization_Type = (PyTypeObject *)PyType_FromSpec(&factor_spec);
	if (!AffineSpace_Type || !SpaceIterGray_Type || !SpaceIterSlow_Type || !Factorization_Type) { Py_DECREF(m); return nullptr; }
	Py_INCREF(AffineSpace_Type); Py_INCREF(SpaceIterGray_Type); Py_INCREF(SpaceIterSlow_Type); Py_INCREF(Factorization_Type);
	QuadGaveUp = PyErr_NewException("_internal.QuadSearchGaveUp", PyExc_RuntimeError, nullptr);
	if (!QuadGaveUp) { Py_DECREF(m); return nullptr; }
	CubicGaveUp = PyErr_NewException("_internal.CubicSearchGaveUp", PyExc_RuntimeError, nullptr);
	if (!CubicGaveUp) { Py_DECREF(m); return nullptr; }
	QuarticGaveUp = PyErr_NewException("_internal.QuarticSearchGaveUp", PyExc_RuntimeError, nullptr);
	if (!QuarticGaveUp) { Py_DECREF(m); return nullptr; }
	Py_INCREF(QuadGaveUp); Py_INCREF(CubicGaveUp); Py_INCREF(QuarticGaveUp);
	if (PyModule_AddObject(m, "QuadSearchGaveUp", QuadGaveUp) < 0 || PyModule_AddObject(m, "CubicSearchGaveUp", CubicGaveUp) < 0 ||
	    PyModule_AddObject(m, "QuarticSearchGaveUp", QuarticGaveUp) < 0 ||
	    PyModule_AddObject(m, "AffineSpace", (PyObject *)AffineSpace_Type) < 0 ||
	    PyModule_AddObject(m, "Factorization", (PyObject *)Factorization_Type) < 0 ||
	    PyModule_AddObject(m, "AffineSpaceIterator", (PyObject *)SpaceIterGray_Type) < 0 ||
	    PyModule_AddObject(m, "AffineSpaceIteratorSlow", (PyObject *)SpaceIterSlow_Type) < 0) {
		Py_DECREF(m);
		return nullptr;
	}
	return m;
}
