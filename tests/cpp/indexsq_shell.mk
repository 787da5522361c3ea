# builds the faiss::IndexScalarQuantizer shell test against the in-tree library:  make -C tests/cpp -f indexsq_shell.mk
# -ffp-contract=off: the shell's host codec must round `vmin + xi * vdiff` twice (include/faiss_amd/IndexScalarQuantizer.h)
ROOT := ../..
CXX  ?= g++
all: test_indexsq_shell
test_indexsq_shell: test_indexsq_shell.cpp $(wildcard $(ROOT)/include/faiss_amd/*.h) $(ROOT)/include/vlq_ivfpq.h
	$(CXX) -std=c++17 -O2 -Wall -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I$(ROOT)/include -I/opt/rocm/include $< -o $@ \
	    -L$(ROOT)/vector_line_quantization_amd/csrc -lvlq_ivfpq -Wl,-rpath,'$$ORIGIN/../../vector_line_quantization_amd/csrc' \
	    -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib
clean:
	rm -f test_indexsq_shell
.PHONY: all clean
