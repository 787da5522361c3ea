# builds the faiss::ScalarQuantizer / faiss::IndexIVFScalarQuantizer shell test against the in-tree library:  make -C tests/cpp -f ivfsq_shell.mk
# -ffp-contract=off: ScalarQuantizer's host arithmetic is the reference's only with one rounding per operation (IndexScalarQuantizer.h)
ROOT := ../..
CXX  ?= g++
all: test_ivfsq_shell
test_ivfsq_shell: test_ivfsq_shell.cpp $(wildcard $(ROOT)/include/faiss_amd/*.h) $(ROOT)/include/vlq_ivfpq.h
	$(CXX) -std=c++17 -O2 -ffp-contract=off -Wall -D__HIP_PLATFORM_AMD__ -I$(ROOT)/include -I/opt/rocm/include $< -o $@ \
	    -L$(ROOT)/vector_line_quantization_amd/csrc -lvlq_ivfpq -Wl,-rpath,'$$ORIGIN/../../vector_line_quantization_amd/csrc' \
	    -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib
clean:
	rm -f test_ivfsq_shell
.PHONY: all clean
