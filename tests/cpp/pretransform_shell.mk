# builds the faiss::IndexPreTransform shell test against the in-tree library:  make -C tests/cpp -f pretransform_shell.mk
ROOT := ../..
CXX  ?= g++
all: test_pretransform_shell
test_pretransform_shell: test_pretransform_shell.cpp $(wildcard $(ROOT)/include/faiss_amd/*.h) $(ROOT)/include/vlq_ivfpq.h
	$(CXX) -std=c++17 -O2 -Wall -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I$(ROOT)/include -I/opt/rocm/include $< -o $@ \
	    -L$(ROOT)/vector_line_quantization_amd/csrc -lvlq_ivfpq -Wl,-rpath,'$$ORIGIN/../../vector_line_quantization_amd/csrc' \
	    -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib
clean:
	rm -f test_pretransform_shell
.PHONY: all clean
