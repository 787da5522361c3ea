# host test of the device buffer's ownership rules (csrc/dev_buf.h) over a counting allocator, under the address and
# undefined-behaviour sanitizers:
#   make -C tests/cpp -f dev_buf.mk
ROOT := ../..
CXX  ?= g++
all: test_dev_buf
test_dev_buf: test_dev_buf.cpp $(ROOT)/vector_line_quantization_amd/csrc/dev_buf.h
	$(CXX) -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -I$(ROOT)/vector_line_quantization_amd/csrc $< -o $@
clean:
	rm -f test_dev_buf
.PHONY: all clean
